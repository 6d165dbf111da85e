"""CPU-only tests (no GPU): the oracle against libtorch's own ops and the reference's constants / KAT, the host logic
(parameter enumeration, step schedule) of the C-ABI library, and that the library exports every declared symbol."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import config as OC, model as OM, pipeline as OP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKENIZER_GOLDEN = os.path.join(ROOT, "tests", "golden", "tokenizer")


@pytest.fixture(scope="module")
def tokdir(tmp_path_factory):
    """the reference's tokenizer/ assets, unpacked from the gzipped copies under tests/golden/tokenizer/ into the same layout
    (clip/bpe_simple_vocab_16e6.txt -- the header and the 48894 merges ClipTokenizer reads --, open_clip/{merges,vocab}.txt, tokenizer.json)"""
    import gzip
    d = tmp_path_factory.mktemp("tokenizer")
    for rel in ("clip/bpe_simple_vocab_16e6.txt", "open_clip/merges.txt", "open_clip/vocab.txt", "tokenizer.json"):
        (d / rel).parent.mkdir(parents=True, exist_ok=True)
        with gzip.open(os.path.join(TOKENIZER_GOLDEN, rel + ".gz"), "rb") as fh:
            (d / rel).write_bytes(fh.read())
    return str(d)


# ------------------------------------------------------------------ oracle primitives vs libtorch (the reference's real backend)
def test_group_norm_matches_libtorch():
    x = torch.randn(2, 64, 5, 7, generator=torch.Generator().manual_seed(0)) * 3 + 1
    g, b = torch.randn(64), torch.randn(64)
    assert torch.allclose(OM.group_norm(x, g, b), F.group_norm(x, 32, g, b, 1e-5), atol=2e-5)


def test_layer_norm_matches_libtorch():
    x = torch.randn(3, 11, 640)
    g, b = torch.randn(640), torch.randn(640)
    assert torch.allclose(OM.layer_norm(x, g, b), F.layer_norm(x, (640,), g, b, 1e-5), atol=2e-5)


def test_silu_gelu_match_libtorch():
    x = torch.linspace(-8, 8, 1001)
    assert torch.allclose(OM.silu(x), F.silu(x), atol=1e-6)
    W = {"p.proj.weight": torch.eye(4), "p.proj.bias": torch.zeros(4)}
    v = torch.randn(5, 4)
    assert torch.allclose(OM.geglu(v, W, "p"), v[:, :2] * F.gelu(v[:, 2:]), atol=1e-6)


@pytest.mark.parametrize("masked", [False, True])
def test_qkv_attention_matches_sdpa(masked):
    # the reference's LibTorch override calls scaled_dot_product_attention (backend.rs:32-79); the generic body the
    # oracle restates (:88-128) must agree with it
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(2, 33, 128, generator=g) for _ in range(3))
    mask = OM.attn_decoder_mask(33) if masked else None
    h = 2
    r = lambda t: t.reshape(2, 33, h, 64).transpose(1, 2)   # noqa: E731
    sdpa = F.scaled_dot_product_attention(r(q), r(k), r(v), attn_mask=mask).transpose(1, 2).flatten(2, 3)
    assert torch.allclose(OM.qkv_attention(q, k, v, mask, h), sdpa, atol=2e-5)


def test_decoder_mask_is_causal():
    m = OM.attn_decoder_mask(4)
    assert m[0, 1] == float("-inf") and m[1, 0] == 0 and m[2, 2] == 0


def test_upsample_matches_interpolate():
    x = torch.randn(1, 3, 4, 5)
    assert torch.equal(OM.upsample_nearest2x(x), F.interpolate(x, scale_factor=2, mode="nearest"))


def test_padded_conv_is_asymmetric_pad():
    x = torch.randn(1, 8, 10, 12)
    W = {"c.weight": torch.randn(8, 8, 3, 3), "c.bias": torch.randn(8)}
    ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), W["c.weight"], W["c.bias"], stride=2)
    assert torch.allclose(OM.padded_conv2d_s2(x, W, "c"), ref, atol=1e-5)


def test_timestep_embedding_layout():
    e = OM.timestep_embedding(torch.tensor([0, 999]), 320)
    assert e.shape == (2, 320)
    assert torch.allclose(e[0, :160], torch.ones(160)) and torch.allclose(e[0, 160:], torch.zeros(160))   # cos | sin
    assert abs(e[1, 0].item() - math.cos(999.0)) < 1e-4


# ------------------------------------------------------------------ constants / schedule the reference fixes
def test_alphas_cumprod_closed_form():
    a = OC.alphas_cumprod()
    assert a.shape == (1000,) and abs(a[999] - 0.00466010) < 1e-6 and abs(a[0] - 0.99915) < 1e-6


def test_step_schedule_matches_reference_loop():
    # (0..1000).rev().step_by(1000 / n): "30 steps" is 31 UNet step pairs (stablediffusion/mod.rs:400-406)
    assert len(OP.step_schedule(30)) == 31 and OP.step_schedule(30)[0] == 999 and OP.step_schedule(30)[-1] == 9
    assert OP.step_schedule(4) == [999, 749, 499, 249]
    assert len(OP.step_schedule(50)) == 50 and len(OP.step_schedule(100)) == 100
    assert OP.step_schedule(50, 800) == list(range(199, -1, -20))


def test_ddim_closed_form_single_step():
    # one step with eps = 0 network: latent' = latent * sqrt(a_prev / a_t)
    cfg = OC.tiny_config()
    W = OM.to_torch(OC.synth_weights(OC.unet_param_specs(cfg)))
    for k in W:
        if k.startswith("conv_out"):
            W[k] = torch.zeros_like(W[k])
    d = OP.Diffuser(cfg, W, OC.alphas_cumprod())
    cond = OP.Conditioning(torch.zeros(3, 128), None, torch.zeros(1, 3, 128), None, torch.zeros(128), None,
                           torch.zeros(1, 128), None, (32, 32))
    x = torch.randn(1, 4, 4, 4)
    out = d.sample_latent(cond, 7.5, 1, x)
    a = OC.alphas_cumprod()
    assert torch.allclose(out, x / math.sqrt(float(a[999])), rtol=1e-5)


def test_param_counts_match_survey():
    n = lambda specs: sum(p.numel for p in specs)   # noqa: E731
    assert abs(n(OC.unet_param_specs(OC.sdxl_base_config())) / 1e6 - 2567.5) < 0.1
    assert abs(n(OC.unet_param_specs(OC.sdxl_refiner_config())) / 1e6 - 2259.5) < 0.1
    assert abs(n(OC.vae_decoder_param_specs(OC.sdxl_vae_config())) / 1e6 - 49.5) < 0.1


def test_block_plan_matches_reference_comment():
    # unet/mod.rs:92-111 lists the base input blocks
    inp, mid, out = OC.unet_block_plan(OC.sdxl_base_config())
    assert [b["kind"] for b in inp] == ["Conv", "Res", "Res", "Down", "ResT", "ResT", "Down", "ResT", "ResT"]
    assert [b.get("c_out", b.get("c")) for b in inp] == [320, 320, 320, 320, 640, 640, 640, 1280, 1280]
    assert [b["c_in"] for b in out] == [2560, 2560, 1920, 1920, 1280, 960, 960, 640, 640]
    assert [b["kind"] for b in out] == ["ResT", "ResT", "ResTU", "ResT", "ResT", "ResTU", "Res", "Res", "Res"]
    assert mid["depth"] == 10 and mid["n_head"] == 20


def test_tokenizer_known_answer_vector(tokdir):
    # the ONE golden vector the reference holds (src/token/clip.rs:236-248), reproduced from its own tokenizer.json
    tokenizers = pytest.importorskip("tokenizers")
    tok = tokenizers.Tokenizer.from_file(tokdir + "/tokenizer.json")
    ids = tok.encode("Hello world! <|startoftext|>asdf<|startoftext|>", add_special_tokens=False).ids
    assert ids == [3306, 1002, 256, 49406, 587, 10468, 49406]


def test_golden_fixture_is_reproducible():
    # committed fixture generated by oracle/make_golden.py from arb_tensor inputs (reference probe recipe)
    path = os.path.join(ROOT, "tests", "golden", "tiny_unet_arb.npz")
    g = np.load(path)
    cfg = OC.tiny_config()
    W = OM.to_torch(OC.synth_weights(OC.unet_param_specs(cfg)))
    out = OM.unet_forward(cfg, W, torch.from_numpy(OC.arb_tensor(1, 4, 8, 8)), torch.tensor([1]),
                          torch.from_numpy(OC.arb_tensor(1, 1, cfg.context_dim)), torch.from_numpy(OC.arb_tensor(1, cfg.adm_in_channels)))
    assert np.allclose(out.numpy(), g["unet_out"], atol=1e-4)


# ------------------------------------------------------------------ C-ABI library: host logic + exported symbols (no compute)
@pytest.fixture(scope="module")
def built(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg


def test_oracle_arithmetic_emulations():
    """oracle.model.NUM (round 5): mode None leaves the fp32 restatement untouched; "f16ref" (the reference's LibTorch<f16> arithmetic, every op
    output an f16 tensor) and "operands" (the engine's f16 mode as the oracle models it: only GEMM operands rounded) on the tiny net.  Checked:
    f16ref outputs ARE f16 values, the hand-written layernorm rounds at each of its seven ops, a single class is never worse than all classes,
    and the class of the reference's own GPU arithmetic is several times wider than the f16-operand model (what the smoke / GPU bounds rest on)."""
    cfg = OC.tiny_config()
    W = OM.to_torch(OC.synth_weights(OC.unet_param_specs(cfg), seed=0))
    g = torch.Generator().manual_seed(5)
    x, t = torch.randn(1, 4, 8, 8, generator=g) * 3, torch.tensor([500])
    c, y = torch.randn(1, 7, cfg.context_dim, generator=g), torch.randn(1, cfg.adm_in_channels, generator=g)
    assert OM.NUM.mode is None
    ref = OM.unet_forward(cfg, W, x, t, c, y)
    try:
        OM.NUM.set("f16ref")
        u = torch.randn(3, 5, 40, generator=g) * 50 + 7
        ln16 = OM.layernorm_fn(u, 1e-5)
        assert torch.equal(ln16, ln16.half().float())
        h = lambda v: v.half().float()      # noqa: E731
        uu = h(u - h(u.mean(-1, keepdim=True)))
        assert torch.equal(ln16, h(uu / h(torch.sqrt(h(h(h(uu * uu).mean(-1, keepdim=True)) + 1e-5)))))
        o16 = OM.unet_forward(cfg, W, x, t, c, y)
        assert torch.equal(o16, o16.half().float()) and torch.isfinite(o16).all()
        e16 = float((o16 - ref).abs().max())
        errs = {}
        for cl in ("qkv", "attn", "out", "xattn", "geglu", "ff", "conv", "conv_res", "conv_skip", "conv_io", "conv_updown", "conv_proj"):
            OM.NUM.set("operands", (cl,))
            errs[cl] = float((OM.unet_forward(cfg, W, x, t, c, y) - ref).abs().max())
        OM.NUM.set("operands", ("qkv", "attn", "out", "xattn", "geglu", "ff", "conv"))
        eall = float((OM.unet_forward(cfg, W, x, t, c, y) - ref).abs().max())
    finally:
        OM.NUM.set(None)
    assert torch.equal(OM.unet_forward(cfg, W, x, t, c, y), ref), "NUM.set(None) must restore the fp32 restatement bit for bit"
    assert all(0 < e <= 1.5 * eall for e in errs.values()), (errs, eall)
    assert max(errs[k] for k in ("conv_res", "conv_skip", "conv_io", "conv_updown", "conv_proj")) <= 1.2 * errs["conv"]
    assert e16 > 2.0 * eall, (e16, eall)      # one rounding per op output costs several times what operand rounding of the GEMMs costs


def test_asm_lint_publication_rule(tmp_path):
    """tools/asm_lint.py rule 5 (round 5): write-through publication stores must be covered by vmcnt(0) before the ticket, and a publishing function
    needs an sc1-load / buffer_inv reader path -- checked on hand-made assembly: the shipped form passes, two broken forms are reported."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("asm_lint", os.path.join(ROOT, "tools", "asm_lint.py"))
    al = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(al)
    good = """kern_good:
\tglobal_store_dwordx4 v[0:1], v[2:5], off sc0 sc1
\ts_nop 1
\ts_waitcnt vmcnt(0)
\tglobal_atomic_add_u32 v6, v[0:1], v7, off sc0
\tglobal_load_dwordx4 v[8:11], v[0:1], off sc1
\ts_endpgm
"""
    bad_wait = good.replace("\ts_waitcnt vmcnt(0)\n", "").replace("kern_good", "kern_no_wait")
    bad_reader = good.replace("off sc1\n\ts_endpgm", "off\n\ts_endpgm").replace("kern_good", "kern_plain_reader")
    for name, text, n in (("good", good, 0), ("bad_wait", bad_wait, 1), ("bad_reader", bad_reader, 1)):
        f = tmp_path / (name + ".s")
        f.write_text(text)
        found = al.lint_publication(str(f))
        assert len(found) == n, (name, found)


def test_asm_lint_scratch_rule(tmp_path):
    """tools/asm_lint.py rule 6 (round 5): a spill inside the matrix loop of a kernel with hand-counted waits is reported; the same spill in the epilogue
    (where the compiler waits for it itself), or in a kernel without inline asm, is not."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("asm_lint", os.path.join(ROOT, "tools", "asm_lint.py"))
    al = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(al)
    mfma = "\tv_mfma_f32_32x32x16_f16 v[0:15], v[16:19], v[20:23], v[0:15]\n"
    asm = "\t;;#ASMSTART\n\tds_read_b128 v[16:19], v24\n\t;;#ASMEND\n"
    spill = "\tscratch_store_dwordx4 off, v[28:31], off offset:16\n"
    cases = {"loop_spill": ("kern_a:\n" + asm + mfma + spill + mfma + "\ts_endpgm\n", 1),
             "epilogue_spill": ("kern_b:\n" + asm + mfma + mfma + spill + "\ts_endpgm\n", 0),
             "no_inline_asm": ("kern_c:\n" + mfma + spill + mfma + "\ts_endpgm\n", 0)}
    for name, (text, n) in cases.items():
        f = tmp_path / (name + ".s")
        f.write_text(text)
        found = al.lint_scratch(str(f))
        assert len(found) == n, (name, found)


def test_shipped_library_kernel_resources(built):
    """tools/kernel_resources.py over the code objects INSIDE the built libsdxl_mi355.so: the kernels with hand-counted wait queues must not use scratch
    (a spill is a VMEM operation).  One known exception, held to its size: the f16 256x160 8-wave tile spills residual fragments in its EPILOGUE (the
    compiler waits for those itself; the asm lint's scratch rule checks that none sits inside its matrix loop).  Every hot kernel keeps the occupancy its
    launch geometry assumes."""
    import importlib.util
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and os.path.exists(os.path.join(llvm, "llvm-readelf"))):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.kernels_of(os.path.join(ROOT, "stable-diffusion-xl-burn_amd", "lib", "libsdxl_mi355.so"))
    assert len(rows) > 80
    hot = [r for r in rows if re.search(r"igemm_pipe_kernel|igemm_wide_kernel|igemm_wreg_kernel|attn_d64", r["name"])]
    assert len(hot) >= 20
    with_scratch = {r["name"]: r["private_segment_fixed_size"] for r in rows if r["private_segment_fixed_size"]}
    allowed = [n for n in with_scratch if "igemm_pipe_kernelILi256ELi160ELi3ELi8ELi8EDF16_" in n]
    assert sorted(with_scratch) == sorted(allowed), with_scratch
    assert all(v <= 128 for v in with_scratch.values()), with_scratch
    for r in hot:
        assert r["vgpr_count"] + r["agpr_count"] <= 512 and kr.waves_per_simd(r) >= 1
        if "igemm_wreg_kernel" in r["name"] or "igemm_pipe_kernelILi256ELi128" in r["name"]:
            assert kr.waves_per_simd(r) >= 2, (r["name"], r["vgpr_count"], r["agpr_count"])     # two workgroups per CU is what their grids are sized for


def test_inline_asm_stores_carry_the_store_data_hazard_nop():
    """An inline-asm VMEM store of more than 64 bits hides the store-data hazard from the compiler (a VALU write of the data registers right behind it
    needs a wait state): every such statement in csrc/ must end with its own s_nop (the first write-through GroupNorm build produced NaNs)."""
    src_dir = os.path.join(ROOT, "stable-diffusion-xl-burn_amd", "csrc")
    found = 0
    for name in sorted(os.listdir(src_dir)):
        if not name.endswith((".hip", ".h", ".cpp")):
            continue
        for m in re.finditer(r'asm volatile\("([^"]*global_store_dwordx[34][^"]*)"', open(os.path.join(src_dir, name)).read()):
            found += 1
            assert "s_nop" in m.group(1), f"{name}: asm store without a hazard nop: {m.group(1)}"
    assert found >= 3


def test_weight_warming_schedule_host_logic(built):
    """WarmSeq::finish (csrc/weights.cpp) on a synthetic UNet-like launch sequence: which entry warms which.  Pure host code behind a test hook
    of the C-ABI library (no device): a transformer block is QKV (pipe kernel, 9.9 MB) / out-projection (weights-in-registers kernel = host, 3.3 MB) /
    packed cross-attention context (0.98 MB, read by the next entry) / fused cross-attention projection (pipe, 3.3 MB) / out-projection (host) /
    GEGLU (pipe, 26 MB) / FF-out (host, 13.1 MB)."""
    l = ctypes.CDLL(built.LIB_PATH)
    MB = 1 << 20
    block = [(9.9, 0), (3.3, 1), (0.98, 0), (3.3, 0), (3.3, 1), (26.3, 0), (13.1, 1)]
    seq = [(29.5, 0), (29.5, 0), (3.3, 1)] + block * 3 + [(3.3, 1), (0.05, 0)]          # convs, proj_in, blocks, proj_out, a tiny conv
    n = len(seq)
    nbytes = (ctypes.c_uint * n)(*[int(b * MB) for b, _ in seq])
    host = (ctypes.c_ubyte * n)(*[h for _, h in seq])
    by = (ctypes.c_int * n)()
    assert l.sdxl_debug_warm_schedule(n, nbytes, host, by) == 0
    by = list(by)
    carried = {}
    for j, h in enumerate(by):
        if h < 0:
            continue
        assert seq[h][1] == 1, "only launches with idle CUs host warming workgroups"
        assert h != j and 1 <= (j - h) % n <= 4, "a host sits at most four entries in front of its target"
        carried.setdefault(h, []).append(j)
    for h, js in carried.items():
        assert len(js) <= 3 and sum(seq[j][0] for j in js) <= 14.0, "three regions, 14 MiB per host"
    for j, (b, h) in enumerate(seq):
        if b > (14.0 if h else 8.0) or b < 0.25:
            assert by[j] < 0, f"entry {j} ({b} MB) must not be a target"
    for k in range(3):                                    # every block: out-projections, context, cross-attention projection and FF-out are warmed
        o = 3 + 7 * k
        assert by[o + 0] < 0 and by[o + 5] < 0            # QKV and GEGLU: too large by rule
        assert by[o + 2] == o + 1 and by[o + 3] == o + 1  # context + cross-attention projection: by the attention out-projection in front of them
        assert by[o + 4] == o + 1                         # the second out-projection too (the projection in between is no host)
        assert by[o + 6] == o + 4                         # FF-out by the cross-attention out-projection
        assert by[o + 1] >= 0                             # the first out-projection: by FF-out of the block in front (proj_in for block 0)
    assert by[3 + 1] == 2 and by[3 + 7 + 1] == 3 + 6
    # degenerate inputs
    one = (ctypes.c_int * 1)()
    assert l.sdxl_debug_warm_schedule(1, (ctypes.c_uint * 1)(4 * MB), (ctypes.c_ubyte * 1)(1), one) == 0 and one[0] == -1


def test_library_exports_every_declared_symbol(built):
    hdr = open(os.path.join(ROOT, "include", "sdxl_mi355.h")).read()
    declared = set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(built.ABI_SYMBOLS), declared ^ set(built.ABI_SYMBOLS)
    l = ctypes.CDLL(built.LIB_PATH)
    for s in declared:
        assert hasattr(l, s), s


def test_no_gpu_is_a_loud_error(built):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(built.EngineError):
        built.Context(0)


@pytest.mark.parametrize("which", ["tiny", "tiny_refiner", "base", "refiner"])
def test_param_specs_equal_oracle(built, which):
    ocfg = {"tiny": OC.tiny_config, "tiny_refiner": OC.tiny_refiner_config, "base": OC.sdxl_base_config,
            "refiner": OC.sdxl_refiner_config}[which]()
    from util import to_pkg_cfg
    mine = built.unet_param_specs(to_pkg_cfg(built, ocfg))
    ref = OC.unet_param_specs(ocfg)
    assert len(mine) == len(ref)
    for a, b in zip(mine, ref):
        assert a.name == b.name and tuple(a.shape) == tuple(b.shape) and a.kind == b.kind
        assert np.float32(a.scale) == b.scale and np.float32(a.mean) == b.mean, a.name


@pytest.mark.parametrize("encoder", [False, True])
def test_vae_param_specs_equal_oracle(built, encoder):
    from util import to_pkg_vcfg
    for v in (OC.tiny_vae_config(), OC.sdxl_vae_config()):
        mine = built.vae_param_specs(to_pkg_vcfg(built, v), encoder)
        ref = OC.vae_encoder_param_specs(v) if encoder else OC.vae_decoder_param_specs(v)
        assert [(a.name, tuple(a.shape), a.kind) for a in mine] == [(b.name, tuple(b.shape), b.kind) for b in ref]
        assert all(np.float32(a.scale) == b.scale for a, b in zip(mine, ref))


def test_step_count_matches_oracle(built):
    for n, s in ((30, 0), (4, 0), (50, 0), (100, 0), (50, 800), (7, 0), (1000, 0)):
        assert built.step_count(n, s) == len(OP.step_schedule(n, s))


def test_bad_config_is_reported(built):
    assert built.lib().sdxl_unet_param_count(ctypes.byref(built.UNetConfig(8, 48, [1, 2], 64, [0, 1], 8).to_c())) == -1
    assert b"head channels" in built.lib().sdxl_last_error()


def test_product_path_never_imports_oracle():
    # the oracle is the checker only: nothing under the package may reference it
    for dirpath, _, files in os.walk(os.path.join(ROOT, "stable-diffusion-xl-burn_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), f


# ------------------------------------------------------------------ Embedder: tokenizers (host string code) + CLIP oracle
@pytest.fixture(scope="module")
def tok(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".tokenizer")


def test_clip_tokenizer_known_answer(tok, tokdir):
    # src/token/clip.rs:236-248 -- the reference's only expected-value test on this path
    t = tok.ClipTokenizer(tokdir)
    text = "Hello world! <|startoftext|>asdf<|startoftext|>"
    ids = t.encode(text, False, False)
    assert ids == [3306, 1002, 256, 49406, 587, 10468, 49406]
    assert t.decode(ids) == "hello world ! <|startoftext|>asdf <|startoftext|>"
    assert (t.start_of_text_token(), t.end_of_text_token(), t.padding_token()) == (49406, 49407, 49407)


def test_tokenizers_agree_with_hf_tokenizer_json(tok, tokdir):
    # the reference ships the HF tokenizer.json of the same vocabulary: an independent implementation to pin against
    tokenizers = pytest.importorskip("tokenizers")
    hf = tokenizers.Tokenizer.from_file(tokdir + "/tokenizer.json")
    clip, oc = tok.ClipTokenizer(tokdir), tok.OpenClipTokenizer(tokdir)
    texts = ["a photo of an astronaut riding a horse on mars", "An elegant bright-colored bird, ultra-detailed 8k!!",
             "  multiple   spaces\tand\nnewlines ", "it's the cat's 1234 toys", "naïve café — déjà vu", "日本語のテキスト", ""]
    for s in texts:
        want = hf.encode(s, add_special_tokens=False).ids
        assert clip.encode(s, False, False) == want, s
        assert oc.encode(s, False, False) == want, s      # same vocabulary, read from files (open_clip.rs:82-113)
    assert oc.padding_token() == 0


def test_tokenize_text_pads_and_truncates(tok, tokdir):
    clip, oc = tok.ClipTokenizer(tokdir), tok.OpenClipTokenizer(tokdir)
    a = tok.tokenize_text("a cat", clip, 77)
    b = tok.tokenize_text("a cat", oc, 77)
    assert len(a) == len(b) == 77 and a[0] == b[0] == 49406
    assert a[:4] == b[:4] and a[3] == 49407 and set(a[4:]) == {49407} and set(b[4:]) == {0}
    long = tok.tokenize_text("cat " * 200, clip, 77)
    assert len(long) == 77 and long[-1] != 49407        # truncation drops the eot, as the reference's loop does


def test_bytes_to_unicode_is_a_bijection(tok):
    bu = tok.bytes_to_unicode()
    assert len(bu) == 256 and len({b for b, _ in bu}) == 256 and len({c for _, c in bu}) == 256
    assert dict(bu)[ord("a")] == "a" and dict(bu)[0] == chr(256) and dict(bu)[32] == chr(256 + 32)


def test_clip_param_counts():
    from oracle import clip as OCL
    n = lambda cfg: sum(p.numel for p in OCL.clip_param_specs(cfg))   # noqa: E731
    assert abs(n(OCL.clip_l_config()) / 1e6 - 123.65) < 0.01            # CLIP ViT-L/14 text tower + projection
    assert abs(n(OCL.open_clip_bigg_config()) / 1e6 - 694.66) < 0.01    # OpenCLIP bigG text tower + projection


def test_clip_oracle_structure():
    from oracle import clip as OCL
    cfg = OCL.tiny_open_clip_config()
    W = OM.to_torch(OC.synth_weights(OCL.clip_param_specs(cfg), 3))
    ids = torch.zeros(2, 77, dtype=torch.int64)
    ids[0, :5] = torch.tensor([49406, 320, 2368, 49407, 0]); ids[1, :7] = torch.tensor([49406, 5, 49407, 9, 49407, 0, 0])
    h0 = OCL.forward_hidden(cfg, W, ids, 0)
    assert torch.equal(h0, W["token_embedding.weight"][ids] + W["position_embedding"][None])
    h, pooled = OCL.forward_hidden_pooled(cfg, W, ids, cfg.n_layer - 1)
    assert torch.allclose(h, OCL.forward_hidden(cfg, W, ids, cfg.n_layer - 1), atol=1e-6)
    assert pooled.shape == (2, cfg.embed_dim)
    # causal: positions before a changed token are unaffected; the pooled row is the FIRST eot (argmax) of each sequence
    ids2 = ids.clone(); ids2[1, 5] = 77
    h2, pooled2 = OCL.forward_hidden_pooled(cfg, W, ids2, cfg.n_layer - 1)
    assert torch.equal(h2[1, :5], h[1, :5]) and not torch.equal(h2[1, 5:], h[1, 5:])
    assert torch.allclose(pooled2, pooled, atol=1e-6)


def test_embedder_oracle_shapes():
    from oracle import clip as OCL
    c1, c2 = OCL.tiny_clip_config(), OCL.tiny_open_clip_config()
    e = OCL.Embedder(c1, OM.to_torch(OC.synth_weights(OCL.clip_param_specs(c1), 1)),
                     c2, OM.to_torch(OC.synth_weights(OCL.clip_param_specs(c2), 2)))
    ids = torch.full((1, 77), 49407, dtype=torch.int64); ids[0, 0] = 49406
    size, crop, ar = torch.tensor([[1024, 1024]]), torch.tensor([[0, 0]]), torch.tensor([1024, 1024])
    c = e.tokens_to_conditioning(ids, ids, ids, ids, size, crop, ar)
    assert c.context_full.shape == (1, 77, c1.n_state + c2.n_state) and c.unconditional_context_full.shape == (77, 320)
    assert c.channel_context.shape == (1, c2.embed_dim + 6 * 256)
    assert c.channel_context_refiner.shape == (1, c2.embed_dim + 5 * 256)


@pytest.mark.parametrize("which", ["tiny_clip", "tiny_open_clip", "clip_l", "open_clip_bigg"])
def test_clip_param_specs_equal_oracle(built, which):
    from oracle import clip as OCL
    ocfg = {"tiny_clip": OCL.tiny_clip_config, "tiny_open_clip": OCL.tiny_open_clip_config, "clip_l": OCL.clip_l_config,
            "open_clip_bigg": OCL.open_clip_bigg_config}[which]()
    mine = built.clip_param_specs(built.CLIPConfig(**ocfg.__dict__))
    ref = OCL.clip_param_specs(ocfg)
    assert len(mine) == len(ref)
    for a, b in zip(mine, ref):
        assert a.name == b.name and tuple(a.shape) == tuple(b.shape) and a.kind == b.kind
        assert np.float32(a.scale) == b.scale and np.float32(a.mean) == b.mean, a.name
    if which == "clip_l":
        assert built.clip_l_config() == built.CLIPConfig(**ocfg.__dict__)
    if which == "open_clip_bigg":
        assert built.open_clip_bigg_config() == built.CLIPConfig(**ocfg.__dict__)


def test_bad_clip_config_is_reported(built):
    assert built.lib().sdxl_clip_param_count(ctypes.byref(built.CLIPConfig(49408, 96, 96, 2, 77, 1, True).to_c())) == -1
    assert b"64 channels per head" in built.lib().sdxl_last_error()


def test_header_is_plain_c_and_links(built, tmp_path):
    # the boundary is a C ABI: the header must compile as C99 (no C++-isms, no torch types) and a C program must link
    # against the library and call the host-only entry points
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text('#include "sdxl_mi355.h"\n'
                   'int main(void) { sdxl_unet_config c; sdxl_clip_config k; sdxl_vae_config v;\n'
                   '  sdxl_unet_config_base(&c); sdxl_clip_config_open_clip_bigg(&k); sdxl_vae_config_default(&v);\n'
                   '  if (sdxl_unet_param_count(&c) <= 0 || sdxl_clip_param_count(&k) != 582) return 2;\n'
                   '  return sdxl_step_count(30, 0, 1000) == 31 ? 0 : 1; }\n')
    exe = tmp_path / "abi"
    libdir = os.path.dirname(built.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", libdir, "-lsdxl_mi355", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_clip_oracle_matches_hf_clip_text_model(act):
    # an independent implementation of the same architecture: HF transformers' CLIPTextModelWithProjection (the model the
    # reference's python/clip.py dumps its CLIP-L weights FROM).  Same random weights through oracle/clip.py must give the
    # same penultimate hidden state and the same pooled, projected embedding.
    transformers = pytest.importorskip("transformers")
    from oracle import clip as OCL
    ocfg = OCL.CLIPConfig(49408, 128, 96, 2, 77, 3, act == "quick_gelu")
    hcfg = transformers.CLIPTextConfig(vocab_size=ocfg.n_vocab, hidden_size=ocfg.n_state, intermediate_size=4 * ocfg.n_state,
                                       num_hidden_layers=ocfg.n_layer, num_attention_heads=ocfg.n_head,
                                       max_position_embeddings=ocfg.n_ctx, hidden_act=act, projection_dim=ocfg.embed_dim,
                                       eos_token_id=2)      # legacy eos id: pooled row = argmax(input_ids), as the reference
    torch.manual_seed(0)
    hf = transformers.CLIPTextModelWithProjection(hcfg).eval()
    sd = {k: v.detach().float() for k, v in hf.state_dict().items()}
    for k in list(sd):                                       # default init is near-degenerate (std 0.02): widen it
        if k.endswith("weight") and sd[k].dim() == 2 and "embedding" not in k:
            sd[k] = sd[k] * 8
    sd = {k: v + (0.05 * torch.randn(v.shape, generator=torch.Generator().manual_seed(len(k))) if k.endswith("bias") else 0) for k, v in sd.items()}
    hf.load_state_dict(sd)
    W = {"token_embedding.weight": sd["text_model.embeddings.token_embedding.weight"],
         "position_embedding": sd["text_model.embeddings.position_embedding.weight"],
         "layer_norm.gamma": sd["text_model.final_layer_norm.weight"], "layer_norm.beta": sd["text_model.final_layer_norm.bias"],
         "text_projection": sd["text_projection.weight"].t().contiguous()}          # save_tensor(text_projection) is [C, E]
    for i in range(ocfg.n_layer):
        h, o = f"text_model.encoder.layers.{i}.", f"blocks.{i}."
        for a, b in (("self_attn.q_proj", "attn.query"), ("self_attn.k_proj", "attn.key"), ("self_attn.v_proj", "attn.value"),
                     ("self_attn.out_proj", "attn.out"), ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
            W[o + b + ".weight"] = sd[h + a + ".weight"].t().contiguous()           # save_linear transposes (save.py:23)
            W[o + b + ".bias"] = sd[h + a + ".bias"]
        for a, b in (("layer_norm1", "attn_ln"), ("layer_norm2", "mlp_ln")):
            W[o + b + ".gamma"], W[o + b + ".beta"] = sd[h + a + ".weight"], sd[h + a + ".bias"]
    for n in [k[:-6] for k in W if k.endswith(".gamma")]:
        W[n + ".eps"] = torch.tensor([hcfg.layer_norm_eps])                         # save_layer_norm writes eps per norm (save.py:31)
    assert set(W) == {p.name for p in OCL.clip_param_specs(ocfg)}
    ids = torch.randint(1, 49000, (2, 77), generator=torch.Generator().manual_seed(1))
    ids[:, 0] = 49406; ids[0, 5] = 49407; ids[0, 6:] = 49407; ids[1, 20] = 49407; ids[1, 21:] = 0
    with torch.no_grad():
        out = hf(input_ids=ids, output_hidden_states=True)
    hid, pooled = OCL.forward_hidden_pooled(ocfg, W, ids, ocfg.n_layer - 1)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())   # noqa: E731
    assert rel(hid, out.hidden_states[-2]) < 5e-5                   # penultimate layer, no final LayerNorm
    assert rel(pooled, out.text_embeds) < 5e-5
    assert rel(OCL.forward_hidden(ocfg, W, ids, ocfg.n_layer), out.hidden_states[-1]) < 5e-5     # fp32 round-off of two different op orders


def test_c_host_example_builds(built, tmp_path):
    # examples/text_to_image.c: tokens -> Embedder -> sample_latent -> latent_to_image in plain C over the ABI (run on the GPU
    # box by hand: 828 ms per 1024^2 image, no Python / torch in the process); here: it compiles and links
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc / HIP headers")
    libdir = os.path.dirname(built.LIB_PATH)
    r = subprocess.run([gcc, "-std=gnu99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "examples", "text_to_image.c"), "-L", libdir, "-lsdxl_mi355",
                        "-L/opt/rocm/lib", "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", "-o", str(tmp_path / "t2i")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_tokenizers_agree_with_hf_on_random_text(tok, tokdir):
    # 300 seeded pseudo-random strings (words, digits, punctuation runs, accents, CJK, emoji, odd spacing) through both
    # tokenizers and the HF tokenizer.json the reference ships
    tokenizers = pytest.importorskip("tokenizers")
    import random
    hf = tokenizers.Tokenizer.from_file(tokdir + "/tokenizer.json")
    clip, oc = tok.ClipTokenizer(tokdir), tok.OpenClipTokenizer(tokdir)
    rng = random.Random(1234)
    words = ["a", "photo", "of", "an", "astronaut", "riding", "horse", "Mars", "ultra-detailed", "8k", "it's", "they'll", "we've",
             "I'm", "don't", "café", "naïve", "über", "日本語", "猫", "🙂", "🚀", "1234", "3.14", "...", "!!!", "?!", "(", ")", "#tag", "@me",
             "under_score", "CamelCase", "x" * 30, "$9.99", "50%", "a/b", "c\\d", "é", "Ω"]
    # (special-token literals are left out on purpose: the reference's regex -- like OpenAI's original -- lets a preceding
    # punctuation run swallow "<|", e.g. "-<|startoftext|>" -> "-<|", "startoftext", "|>", whereas HF extracts added tokens
    # before pre-tokenisation; tokenizer.py follows the reference, and the KAT above covers the special tokens)
    seps = [" ", "  ", "\t", "\n", " , ", "-", ""]
    for _ in range(300):
        s = "".join(rng.choice(words) + rng.choice(seps) for _ in range(rng.randint(1, 12)))
        want = hf.encode(s, add_special_tokens=False).ids
        assert clip.encode(s, False, False) == want, repr(s)
        assert oc.encode(s, False, False) == want, repr(s)


def test_special_token_literal_follows_the_reference_regex(tok, tokdir):
    # src/token/clip.rs:110: the alternation is tried left to right at each position, so a punctuation run that starts
    # BEFORE "<|startoftext|>" takes the "<|" with it (OpenAI's original behaves the same; HF's added-token pass does not)
    t = tok.ClipTokenizer(tokdir)
    assert t.encode("a <|startoftext|>", False, False) == [320, 49406]
    ids = t.encode("-<|startoftext|>", False, False)
    assert 49406 not in ids and t.decode(ids).replace(" ", "") == "-<|startoftext|>"


def _ref_dump(name):
    import numpy as np
    f = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref", name + ".npy")
    return np.load(f) if os.path.exists(f) else None


def test_oracle_matches_reference_dumps():
    """Golden vectors produced by the REAL reference (oracle/_ref_recipe: its loaders + UNet / Encoder / Decoder forwards on the
    arb_tensor probes of src/bin/test/main.rs:51-54,128-162, run on a box with cargo) pin the oracle when they are committed under
    tests/golden/ref/.  Until then the oracle stays "parity unpinned" and this test skips."""
    import numpy as np
    import pytest
    import torch
    from oracle import config as OC, model as OM
    got = {k: _ref_dump(k) for k in ("unet_out", "encoder_out", "decoder_out")}
    if all(v is None for v in got.values()):
        pytest.skip("no reference dumps committed (tests/golden/ref/ is empty): see oracle/_ref_recipe/README.md")
    ucfg, vcfg = OC.tiny_config(), OC.tiny_vae_config()
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())   # noqa: E731
    if got["unet_out"] is not None:
        W = OM.to_torch(OC.synth_weights(OC.unet_param_specs(ucfg), 0))
        out = OM.unet_forward(ucfg, W, torch.from_numpy(OC.arb_tensor(1, 4, 8, 8)), torch.tensor([1]),
                              torch.from_numpy(OC.arb_tensor(1, 1, ucfg.context_dim)), torch.from_numpy(OC.arb_tensor(1, ucfg.adm_in_channels)))
        assert rel(out.numpy().reshape(-1), got["unet_out"].reshape(-1)) < 1e-5
    if got["encoder_out"] is not None:
        W = OM.to_torch(OC.synth_weights(OC.vae_encoder_param_specs(vcfg), 0))
        out = OM.vae_encoder_forward(vcfg, W, torch.from_numpy(OC.arb_tensor(1, 3, 16, 16)))
        assert rel(out.numpy().reshape(-1), got["encoder_out"].reshape(-1)) < 1e-5
    if got["decoder_out"] is not None:
        W = OM.to_torch(OC.synth_weights(OC.vae_decoder_param_specs(vcfg), 0))
        out = OM.vae_decoder_forward(vcfg, W, torch.from_numpy(OC.arb_tensor(1, 4, 4, 4)))
        assert rel(out.numpy().reshape(-1), got["decoder_out"].reshape(-1)) < 1e-5


def test_ref_recipe_exports_the_reference_tree(tmp_path):
    """the pin recipe's exporter writes what the reference's loaders read (python/save.py conventions): spot checks"""
    import numpy as np
    from oracle._ref_recipe import export_params as EP
    EP.main(str(tmp_path))
    rd = lambda *p: np.load(os.path.join(str(tmp_path), *p))   # noqa: E731
    assert rd("params_unet", "input_blocks", "0", "stride.npy").tolist() == [2.0, 1.0, 1.0]          # [len, values]: (1, 1)
    assert rd("params_unet", "input_blocks", "0", "n_channels_in.npy").tolist() == [1.0, 4.0]
    assert rd("params_vae", "encoder", "n_block.npy").tolist() == [1.0, 4.0]
    assert rd("params_vae", "encoder", "blocks", "0", "downsampler", "padding.npy").tolist() == [4.0, 0.0, 1.0, 0.0, 1.0]
    assert rd("params_vae", "encoder", "blocks", "0", "downsampler", "conv", "stride.npy").tolist() == [2.0, 2.0, 2.0]
    assert rd("params_vae", "decoder", "norm_out", "n_group.npy").tolist() == [1.0, 32.0]


def test_production_gemm_assembly_has_no_async_read_hazard(tmp_path):
    """tools/asm_lint.py over the device assembly of the production GEMM translation unit: no instruction may read or overwrite the
    destination registers of a hand-written asynchronous `ds_read_b128` before a counted `s_waitcnt lgkmcnt` covers it.  (The compiler
    believes an inline-asm output complete when the statement ends; it broke the split-operand kernel exactly this way when that kernel
    grew a second copy of its k-loop.)  Takes about two minutes of hipcc."""
    import shutil
    import subprocess
    import sys
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import asm_lint
    src = os.path.join(ROOT, "stable-diffusion-xl-burn_amd", "csrc", "igemm_glds.hip")
    out = str(tmp_path / "igemm_glds.s")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "--cuda-device-only", "-S", src, "-o", out,
                        "-Wno-unused-function"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    findings = asm_lint.lint(out) + asm_lint.lint_publication(out) + asm_lint.lint_scratch(out)
    assert not findings, "\n".join(findings[:10])
    # the lint must see the kernels it is meant to check
    text = open(out).read()
    assert text.count("ds_read_b128") > 500 and "igemm_pipe_kernel" in text
    # the attention translation unit (raw barriers, LDS-DMA rings, hand-counted vmcnt waits) under the same rules
    src2, out2 = os.path.join(ROOT, "stable-diffusion-xl-burn_amd", "csrc", "attention.hip"), str(tmp_path / "attention.s")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "--cuda-device-only", "-S", src2, "-o", out2,
                        "-Wno-unused-function"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    findings = asm_lint.lint(out2) + asm_lint.lint_publication(out2) + asm_lint.lint_scratch(out2)
    assert not findings, "\n".join(findings[:10])
    assert "attn_d64_mix_kernel" in open(out2).read()


def test_weights_in_registers_gemm_assembly_has_no_async_load_hazard(tmp_path):
    """the same lint over igemm_wreg.hip, plus its VM-queue rule: the weight fragments are inline-asm `global_load_dwordx4` with
    hand-counted `s_waitcnt vmcnt`, so no instruction may touch a fragment register between its load and the wait that covers it (a
    128-row build of this kernel spilled in-flight fragment registers to scratch -- wrong results on the GPU, four findings here)."""
    import shutil
    import subprocess
    import sys
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import asm_lint
    src, out = os.path.join(ROOT, "stable-diffusion-xl-burn_amd", "csrc", "igemm_wreg.hip"), str(tmp_path / "igemm_wreg.s")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "--cuda-device-only", "-S", src, "-o", out,
                        "-Wno-unused-function"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    findings = asm_lint.lint(out) + asm_lint.lint_vm(out) + asm_lint.lint_scratch(out)
    assert not findings, "\n".join(findings[:10])
    text = open(out).read()
    assert "igemm_wreg_kernel" in text and text.count("global_load_dwordx4") > 100 and ".vgpr_spill_count: 0" in text
    # the kernels must keep two waves per SIMD (<= 256 registers) without spilling
    import re
    for m in re.finditer(r"\.name:\s+(\S*igemm_wreg_kernel\S*).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", text, re.S):
        assert int(m.group(2)) <= 256 and int(m.group(3)) == 0, m.group(0)[:200]
