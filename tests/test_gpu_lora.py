"""Create-time adapters on the GPU: the merge op against fp64, the adapter source against the op in every packing form, the adapted models
against the oracle on merged weights, the f16-parameter modes with and without SDXL_LORA_ROUND_F16, the Diffuser, and the error paths.
Tiny configurations at 16 x 16; the oracle references are computed once per module."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import config as OC, model as OM, pipeline as OP
from util import max_abs, rel_err, seeded, to_pkg_cfg, unet_weights
from test_gpu_models import FWD_TOL, F16W_CLASSES, LAT_ABS_F32, MIX_CLASSES, _cond, _pkg_cond
import lora_ref as LR

pytestmark = pytest.mark.gpu

# adapter strength of the model tests (lora_ref.adapter_set): each adapted layer gets a branch about as strong as its base layer.  Measured with the
# oracle alone: the merged tiny UNet's output then differs from the base output by 0.67 (tiny) / 0.68 (tiny refiner) in rel_err's measure,
# 150 x FWD_TOL[1] -- a tolerance the unadapted model would meet as well shows nothing, so the tests below assert >= 100 x.
MAGNITUDE = 1.0
F16W7_CLASSES = 4096 | 512 | 256      # SDXL_DTYPE_F32_SPLIT_F16W in full (test_gpu_models.py)


def _entries(pkg, adapters):
    return [pkg.lora_entry(i, down, up, alpha, strength) for i, down, up, alpha, strength in adapters]


def _reference_flat(pkg, ctx, specs, flat, entries, flags=0):
    """the flat weights with every entry merged by the OP (sdxl_lora_merge) in the order given; flags go with the last entry of each tensor"""
    offs = np.concatenate([[0], np.cumsum([int(np.prod(p.shape)) for p in specs])])
    out = np.array(flat, dtype=np.float32, copy=True)
    last = {e.param_index: k for k, e in enumerate(entries)}
    for k, e in enumerate(entries):
        p = specs[e.param_index]
        seg = out[offs[e.param_index]:offs[e.param_index + 1]]
        w = torch.from_numpy(seg.copy()).reshape(p.shape[0], -1).cuda()
        seg[:] = pkg.lora_merge(ctx, w, e.keep[0], e.keep[1], e.scale, flags if last[e.param_index] == k else 0).cpu().numpy().reshape(-1)
    return out


class Tiny:
    def __init__(self, pkg, ocfg):
        self.ocfg, self.cfg = ocfg, to_pkg_cfg(pkg, ocfg)
        self.specs = pkg.unet_param_specs(self.cfg)
        self.W = unet_weights(ocfg)
        self.flat = pkg.flatten_weights(self.specs, {k: v.numpy() for k, v in self.W.items()})
        self.adapters = LR.adapter_set(self.specs, MAGNITUDE)
        B = 2
        self.x = torch.from_numpy(OC.arb_tensor(B, 4, 16, 16))
        self.context = torch.from_numpy(OC.arb_tensor(B, 5, ocfg.context_dim))
        self.y = torch.from_numpy(OC.arb_tensor(B, ocfg.adm_in_channels))
        self.t = torch.tensor([999, 1], dtype=torch.int32)

    def oracle(self, W):
        return OM.unet_forward(self.ocfg, W, self.x, self.t.long(), self.context, self.y)

    def forwards(self, u, n=3):      # eager, capture, replay
        return [u.forward(self.x.cuda(), self.t.cuda(), self.context.cuda(), self.y.cuda()).cpu() for _ in range(n)]


@pytest.fixture(scope="module")
def tiny(pkg):
    return Tiny(pkg, OC.tiny_config())


@pytest.fixture(scope="module")
def oracle_refs(tiny):
    """(base output, output on the fp64-merged weights) of the oracle"""
    return tiny.oracle(tiny.W), tiny.oracle(LR.merged_fp64(tiny.specs, tiny.W, tiny.adapters))


# ---------------------------------------------------------------------------------------------------------------- 1. the op
@pytest.mark.parametrize("scale", [1.0, -0.37])
@pytest.mark.parametrize("rows,cols,rank", [(1, 1, 1), (37, 53, 3), (64, 64, 16), (130, 257, 17), (96, 576, 33), (257, 64, 64)])
def test_merge_op_against_fp64(pkg, ctx, rows, cols, rank, scale):
    # tails in both dimensions of the 16 x 64 tile, rank-chunk boundaries on either side of 16 / 32 / 64.  Bound from the fixed arithmetic
    # (acc = fma chain over j ascending, w = fma(scale, acc, w)): (rank + 2) 2^-24 (|w| + |scale| sum_j |left||right|) + one fp32 ulp
    w, left, right = seeded(rows, cols, seed=rows), seeded(rows, rank, seed=cols + 1000), seeded(rank, cols, seed=rank + 2000)
    out = pkg.lora_merge(ctx, w.cuda(), left.cuda(), right.cuda(), scale).cpu()
    ref, bound = LR.merge_bound(w, left, right, float(np.float32(scale)))
    err = (out.double() - ref).abs()
    print(f"lora_merge {rows}x{cols} rank {rank} scale {scale}: max err {err.max():.3e}, worst err / bound {(err / bound).max():.3f}")
    assert bool((err <= bound).all())
    assert not torch.equal(out, w)
    again = pkg.lora_merge(ctx, w.cuda(), left.numpy(), right.numpy(), scale).cpu()      # host arrays this time: staged by the source
    assert torch.equal(again.view(torch.int32), out.view(torch.int32)), "two runs differ"
    zero = pkg.lora_merge(ctx, w.cuda(), left.cuda(), right.cuda(), 0.0).cpu()
    assert torch.equal(zero.view(torch.int32), w.view(torch.int32)), "scale 0 changed w"
    r16 = pkg.lora_merge(ctx, w.cuda(), left.cuda(), right.cuda(), scale, pkg.LORA_ROUND_F16).cpu()
    assert torch.equal(r16.view(torch.int32), out.half().float().view(torch.int32)), "SDXL_LORA_ROUND_F16 is not float(half(x)) of the plain result"


# ---------------------------------------------------------------------------------------------------------------- 2. the source is the op
@pytest.mark.parametrize("dtype", [0, 1, 3, 4])
def test_adapter_source_equals_the_op_in_every_packing(pkg, ctx, tiny, dtype):
    # fused QKV (attn1.query twice + attn1.value), hoisted context K / V (attn2.key, attn2.value), GEGLU and FF-out, a 3x3 and a 1x1 convolution,
    # proj_in, the GEMV time embedding and the fused ResBlock embedding projection: UNet(lora=...) must be the UNet built from flat weights the
    # op merged, bit for bit, over eager / capture / replay
    entries = _entries(pkg, tiny.adapters)
    assert len({e.param_index for e in entries}) == len(entries) - 1      # exactly one tensor adapted twice
    u = pkg.UNet(ctx, tiny.cfg, dtype, seed=0, lora=entries)
    ref = pkg.UNet(ctx, tiny.cfg, dtype, weights=_reference_flat(pkg, ctx, tiny.specs, tiny.flat, entries))
    outs, refs = tiny.forwards(u), tiny.forwards(ref)
    base = tiny.forwards(pkg.UNet(ctx, tiny.cfg, dtype, seed=0), 1)[0]
    print(f"dtype {dtype}: lora vs op-merged flat weights max diff {max_abs(outs[0], refs[0]):.3e}; adapter moves the output by {rel_err(outs[0], base):.3f}")
    assert rel_err(outs[0], base) > 100 * FWD_TOL[1]
    for o in outs + refs:
        assert torch.equal(o, refs[0])


@pytest.mark.parametrize("dtype", [0, 1, 3, 4])
def test_no_entries_equals_the_plain_constructor(pkg, ctx, tiny, dtype):
    plain, empty = pkg.UNet(ctx, tiny.cfg, dtype, seed=0), pkg.UNet(ctx, tiny.cfg, dtype, seed=0, lora=[])
    assert plain.weight_arena()[1] == empty.weight_arena()[1] and plain.mix_classes() == empty.mix_classes()
    a, b = tiny.forwards(plain), tiny.forwards(empty)
    assert all(torch.equal(o, a[0]) for o in a + b)


def test_every_base_takes_adapters(pkg, ctx, tiny):
    # the three bases of sdxl_unet_create_lora: flat fp32, flat f16 (adapters land on the widened values), the synthetic seed
    entries = _entries(pkg, tiny.adapters)
    offs = np.concatenate([[0], np.cumsum([int(np.prod(p.shape)) for p in tiny.specs])])
    flat16 = tiny.flat.astype(np.float16)
    f32_of_16 = flat16.astype(np.float32)
    for i, p in enumerate(tiny.specs):
        if p.kind == 5:
            f32_of_16[offs[i]] = tiny.flat[offs[i]]      # the f16 image of the default eps stands for the default (FlatSourceF16)
    for base, ref_flat in ((dict(weights=tiny.flat), tiny.flat), (dict(weights=flat16), f32_of_16), (dict(seed=0), tiny.flat)):
        u = pkg.UNet(ctx, tiny.cfg, 1, lora=entries, **base)
        ref = pkg.UNet(ctx, tiny.cfg, 1, weights=_reference_flat(pkg, ctx, tiny.specs, ref_flat, entries))
        assert torch.equal(tiny.forwards(u, 1)[0], tiny.forwards(ref, 1)[0]), list(base)


# ---------------------------------------------------------------------------------------------------------------- 3. against the oracle
def test_the_adapter_matters_to_the_oracle(oracle_refs):
    base, merged = oracle_refs
    moved = rel_err(merged, base)
    print(f"oracle: merged vs base output {moved:.3f} (100 x FWD_TOL[1] = {100 * FWD_TOL[1]:.3f})")
    assert moved >= 100 * FWD_TOL[1]


@pytest.mark.parametrize("dtype", [0, 1, 3])
def test_adapted_unet_against_the_oracle(pkg, ctx, tiny, oracle_refs, dtype):
    base, merged = oracle_refs
    assert rel_err(merged, base) >= 100 * FWD_TOL[1], "the adapter does not matter: the tolerance below would show nothing"
    u = pkg.UNet(ctx, tiny.cfg, dtype, seed=0, lora=_entries(pkg, tiny.adapters))
    outs = tiny.forwards(u)
    e = rel_err(outs[0], merged)
    print(f"adapted unet_forward dtype={dtype}: rel err {e:.3e} (vs the BASE oracle output: {rel_err(outs[0], base):.3f})")
    assert e < FWD_TOL[dtype]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


# ---------------------------------------------------------------------------------------------------------------- 4. f16-parameter modes
@pytest.fixture(scope="module")
def tiny16(tiny):
    """the f16-valued weights SDXL_SEED_F16_WEIGHTS generates, and the oracle's base output on them"""
    W16 = {k: (v if k.endswith(".eps") else v.half().float()) for k, v in tiny.W.items()}
    return W16, tiny.oracle(W16)


@pytest.mark.parametrize("dtype,fallback_dtype,fallback_classes,full_classes", [(5, 4, MIX_CLASSES, F16W_CLASSES), (7, 3, 0, F16W7_CLASSES)])
def test_f16_parameter_modes_with_an_adapter(pkg, ctx, tiny, tiny16, dtype, fallback_dtype, fallback_classes, full_classes):
    W16, base16 = tiny16
    adapters = LR.adapter_set(tiny.specs, 2.0, rows=LR.ADAPTERS[:1])      # attn1.query alone, twice the strength
    entries = _entries(pkg, adapters)
    e = entries[0]
    name = tiny.specs[e.param_index].name
    assert name.endswith(".attn1.query.weight")
    seed = pkg.SEED_F16_WEIGHTS
    assert pkg.UNet(ctx, tiny.cfg, dtype, seed=seed).mix_classes() == full_classes
    # merged tensors are not f16 values: the mode falls back like on any such checkpoint, to the bits of its fallback dtype
    u = pkg.UNet(ctx, tiny.cfg, dtype, seed=seed, lora=entries)
    assert u.mix_classes() == fallback_classes
    uf = pkg.UNet(ctx, tiny.cfg, fallback_dtype, seed=seed, lora=entries)
    assert torch.equal(tiny.forwards(u, 1)[0], tiny.forwards(uf, 1)[0])
    # SDXL_LORA_ROUND_F16: the adapted tensor is an f16 tensor again, the mode keeps its classes
    ur = pkg.UNet(ctx, tiny.cfg, dtype, seed=seed, lora=entries, lora_flags=pkg.LORA_ROUND_F16)
    assert ur.mix_classes() == full_classes
    Wr = dict(W16)
    wq = pkg.lora_merge(ctx, W16[name].cuda(), e.keep[0], e.keep[1], e.scale, pkg.LORA_ROUND_F16).cpu()
    assert torch.equal(wq, wq.half().float()) and not torch.equal(wq, W16[name])
    Wr[name] = wq
    ref = tiny.oracle(Wr)
    assert rel_err(ref, base16) > 10 * FWD_TOL[5], "the adapter does not matter"
    outs = tiny.forwards(ur)
    err = rel_err(outs[0], ref)
    print(f"dtype {dtype} + ROUND_F16 adapter: rel err {err:.3e}; adapter moves the oracle output by {rel_err(ref, base16):.3f}")
    assert err < FWD_TOL[dtype]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


# ---------------------------------------------------------------------------------------------------------------- 5. Diffuser
def test_diffuser_with_adapters(pkg, ctx, tiny):
    res = (128, 128)      # 16 x 16 latents
    c, oc = _cond(tiny.ocfg, 1, res)
    noise = seeded(1, 4, 16, 16, seed=40)
    Wm = LR.merged_fp64(tiny.specs, tiny.W, tiny.adapters)
    ref = OP.Diffuser(tiny.ocfg, Wm, OC.alphas_cumprod()).sample_latent(oc, 7.5, 4, noise)
    d = pkg.Diffuser(ctx, tiny.cfg, 0, seed=0, lora=_entries(pkg, tiny.adapters))
    out = d.sample_latent(_pkg_cond(pkg, c, res), 7.5, 4, noise.cuda()).cpu()
    plain = pkg.Diffuser(ctx, tiny.cfg, 0, seed=0).sample_latent(_pkg_cond(pkg, c, res), 7.5, 4, noise.cuda()).cpu()
    e = max_abs(out, ref)
    print(f"Diffuser(lora=) 4 steps CFG 7.5: latent max-abs err {e:.3e} (|latent| max {ref.abs().max():.2f}; unadapted engine: {max_abs(plain, ref):.3e})")
    assert max_abs(plain, ref) > 100 * LAT_ABS_F32, "the adapter does not matter"
    assert np.isfinite(e) and e < LAT_ABS_F32


def test_refiner_diffuser_with_adapters(pkg, ctx):
    r = Tiny(pkg, OC.tiny_refiner_config())
    res = (128, 128)
    c, oc = _cond(r.ocfg, 1, res, refiner=True)
    latent, noise = seeded(1, 4, 16, 16, seed=41), seeded(1, 4, 16, 16, seed=42)
    step_start, n_steps = 920, 25      # two iterations (t = 79, 39)
    assert pkg.step_count(n_steps, step_start) == 2
    Wm = LR.merged_fp64(r.specs, r.W, r.adapters)
    ref = OP.Diffuser(r.ocfg, Wm, OC.alphas_cumprod()).refine_latent(latent, oc, 7.5, step_start, n_steps, noise)
    d = pkg.Diffuser(ctx, r.cfg, 0, seed=0, lora=_entries(pkg, r.adapters))
    out = d.refine_latent(latent.cuda(), _pkg_cond(pkg, c, res, True), 7.5, step_start, n_steps, noise.cuda()).cpu()
    plain = pkg.Diffuser(ctx, r.cfg, 0, seed=0).refine_latent(latent.cuda(), _pkg_cond(pkg, c, res, True), 7.5, step_start, n_steps, noise.cuda()).cpu()
    e = max_abs(out, ref)
    print(f"refiner Diffuser(lora=) refine_latent: max-abs err {e:.3e} (unadapted engine: {max_abs(plain, ref):.3e})")
    assert max_abs(plain, ref) > 100 * LAT_ABS_F32, "the adapter does not matter"
    assert e < LAT_ABS_F32


# ---------------------------------------------------------------------------------------------------------------- 6. errors
def test_create_lora_argument_errors_leave_everything_usable(pkg, ctx, tiny):
    l = pkg.lib()
    c = tiny.cfg.to_c()
    good = _entries(pkg, tiny.adapters)
    arr = (pkg.LoraEntry * len(good))(*good)
    flat = np.ascontiguousarray(tiny.flat)
    flat16 = tiny.flat.astype(np.float16)
    p32, p16 = flat.ctypes.data_as(ctypes.c_void_p), flat16.ctypes.data_as(ctypes.c_void_p)
    bad = (pkg.LoraEntry * len(good))(*good)
    bad[3].rank = 0
    sentinel = 0x5eed0
    cases = {"both bases": (p32, p16, arr, 0, "exactly one base"), "bad entry": (p32, None, bad, 0, "entry 3"), "unknown flags": (None, None, arr, 2, "flag")}
    for what, (w32, w16, entries, flags, word) in cases.items():
        h = ctypes.c_void_p(sentinel)
        rc = l.sdxl_unet_create_lora(ctx.h, ctypes.byref(c), 0, w32, w16, ctypes.c_uint64(0), entries, len(good), flags, ctypes.byref(h))
        assert rc == 1 and h.value == sentinel and word in l.sdxl_last_error().decode(), (what, rc, l.sdxl_last_error())
        hd = ctypes.c_void_p(sentinel)
        a = np.ascontiguousarray(pkg.default_alphas_cumprod())
        rc = l.sdxl_diffuser_create_lora(ctx.h, ctypes.byref(c), 0, w32, w16, ctypes.c_uint64(0), entries, len(good), flags,
                                         a.ctypes.data_as(ctypes.c_void_p), int(a.shape[0]), ctypes.byref(hd))
        assert rc == 1 and hd.value == sentinel, what
    with pytest.raises(pkg.InvalidArgument):
        pkg.UNet(ctx, tiny.cfg, 0, seed=0, lora=good, lora_flags=4)
    wrong = pkg.lora_entry(good[0].param_index, np.zeros((2, 7), np.float32), np.zeros((5, 2), np.float32))      # extents of another tensor
    with pytest.raises(pkg.EngineError):
        pkg.UNet(ctx, tiny.cfg, 0, seed=0, lora=[wrong])
    for args in ((0, 4, 1), (4, 0, 1)):      # the op: empty tensors are refused as well
        assert l.sdxl_lora_merge(ctx.h, None, ctypes.c_void_p(256), args[0], args[1], p32, p32, args[2], ctypes.c_float(1.0), 0) == 1
    # the context is as usable as before: a plain create and forward
    u = pkg.UNet(ctx, tiny.cfg, 0, seed=0)
    ref = pkg.UNet(ctx, tiny.cfg, 0, weights=tiny.flat)
    assert torch.equal(tiny.forwards(u, 1)[0], tiny.forwards(ref, 1)[0])
