"""The UNet's conditioning path op by op: gemv_kernel behind launch_gemv (sdxl_gemv: time / label embedding MLPs, the hoisted lin_embed(silu(emb)))
and temb_kernel (sdxl_timestep_embedding) against fp64 references with derived per-element bounds (tests/gemv_ref.py), at the shapes where the
kernel takes another path: k-loops of 1 / 2.5 / 5.5 / 32 iterations, K and N tails, cols = 4 with a partial last block, the launcher's row chunks
(5+1, 5+3, 6+1, 8+1, 1+1) and its 64 KiB limit.  tests/test_cpu_gemv_ref.py shows, on these operands, that a subtly wrong kernel leaves the bounds.
Then the same path inside a model: a tiny UNet whose label MLP is as wide as SDXL-base's (K = 2816), a batch of 8, against the oracle per entry.

Every assertion prints its worst error / bound first (pytest -s; recorded in profiles/conditioning_path_tests.txt)."""
import dataclasses

import numpy as np
import pytest
import torch

import gemv_ref as R
from oracle import config as OC, model as OM
from test_gpu_models import FWD_TOL, weights_for
from util import rel_err, to_pkg_cfg

pytestmark = pytest.mark.gpu

DTYPES = {0: "f32", 1: "f16", 3: "f32_split"}      # SDXL_DTYPE_F32, _F16, _F32_SPLIT (fp32 GEMV weights, as a split-operand UNet packs them)

_refs = {}


def _case(name, f16):
    """(operands, fp64 reference, bound) of a gemv_ref.GEMV_CASES row: computed once, shared by the dtypes and tests, never modified"""
    if (name, f16) not in _refs:
        _, K, N, Bm, flags = next(c for c in R.GEMV_CASES if c[0] == name)
        d = R.make_case(K, N, Bm, flags, f16)
        _refs[(name, f16)] = (d, *R.gemv_ref(**d))
    return _refs[(name, f16)]


def _run(pkg, ctx, d, dtype, rows=None, out=None):
    """pkg.gemv on the operands of a case (rows: a slice of the batch entries)"""
    rows = slice(None) if rows is None else rows
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return pkg.gemv(ctx, dev(d["x"][rows]), dev(d["w"]), dev(d["bias"]), None if d["yadd"] is None else dev(d["yadd"][rows]),
                    silu_in=d["silu_in"], silu_out=d["silu_out"], dtype=dtype, out=out)


def _ratio(out, y, bound):
    return float((np.abs(out.double().cpu().numpy() - y) / bound).max())


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", [c[0] for c in R.GEMV_CASES])
def test_gemv_within_derived_bound(pkg, ctx, name, dtype):
    d, y, bound = _case(name, dtype == pkg.DTYPE_F16)
    out = _run(pkg, ctx, d, dtype)
    assert out.shape == y.shape and torch.isfinite(out).all()
    r = _ratio(out, y, bound)
    print(f"gemv {name} K={d['x'].shape[1]} N={d['w'].shape[1]} Bm={d['x'].shape[0]} {DTYPES[dtype]}: worst error / bound {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_gemv_refuses_k_beyond_the_staging_limit(pkg, ctx, dtype):
    # K = 16385 needs more than 64 KiB for one staged row: the launcher throws before any launch; the context stays usable
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(1, 16385, generator=g).cuda(), torch.randn(16385, 8, generator=g).cuda()
    with pytest.raises(pkg.EngineError, match="64 KiB"):
        pkg.gemv(ctx, x, w, dtype=dtype)
    d, y, bound = _case("k_and_n_tails", dtype == pkg.DTYPE_F16)
    assert _ratio(_run(pkg, ctx, d, dtype), y, bound) <= 1.0


def test_gemv_refuses_other_dtypes_and_timestep_embedding_odd_dims(pkg, ctx):
    d, _, _ = _case("k_and_n_tails", False)
    for dtype in (pkg.DTYPE_F16_F32RES, pkg.DTYPE_F32_SPLIT_MIX, pkg.DTYPE_F32_SPLIT_F16W, 99):
        with pytest.raises(pkg.EngineError):
            _run(pkg, ctx, d, dtype)
    with pytest.raises(pkg.EngineError):
        pkg.timestep_embedding(ctx, torch.tensor([1.0]).cuda(), 65)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_gemv_entries_are_independent_across_the_chunk_boundary(pkg, ctx, dtype):
    # K = 2816: 5 rows per launch, so entries 0 and 4 of a batch of 8 come out of the first launch, 5 and 7 out of the second (offset X / Y / Yadd):
    # each is bit-identical to the same entry run alone
    d, y, bound = _case("all_flags_null_bias_two_launches", dtype == pkg.DTYPE_F16)
    assert d["yadd"] is not None and d["x"].shape == (8, 2816)
    both = _run(pkg, ctx, d, dtype)
    assert _ratio(both, y, bound) <= 1.0
    for b in (0, 4, 5, 7):
        alone = _run(pkg, ctx, d, dtype, rows=slice(b, b + 1))
        assert torch.equal(alone[0], both[b]), b


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_gemv_leaves_the_rows_after_the_batch_alone(pkg, ctx, dtype):
    d, y, bound = _case("all_flags_null_bias_two_launches", dtype == pkg.DTYPE_F16)
    Bm, N = y.shape
    buf = torch.full((Bm + 2, N), float("nan"), device="cuda")
    out = _run(pkg, ctx, d, dtype, out=buf)
    assert out.data_ptr() == buf.data_ptr() and out.shape == (Bm, N)
    assert torch.isnan(buf[Bm:]).all(), "the second launch wrote past row Bm - 1"
    assert _ratio(buf[:Bm], y, bound) <= 1.0


@pytest.mark.parametrize("n", [8, 1])
@pytest.mark.parametrize("dim", R.TEMB_DIMS)
def test_timestep_embedding_within_derived_bound(pkg, ctx, dim, n):
    t = np.asarray(R.TEMB_T if n == 8 else R.TEMB_T[2:3], np.float32)
    ref, bound = R.temb_ref(t, dim)
    out = pkg.timestep_embedding(ctx, torch.from_numpy(t).cuda(), dim)
    assert out.shape == ref.shape
    r = _ratio(out, ref, bound)
    print(f"timestep_embedding dim={dim} n={n}: worst error / bound {r:.4f}")
    assert r <= 1.0
    if n == 8:      # t = 0: cos(0) = 1 and sin(0) = 0, exactly
        assert t[0] == 0.0 and (out[0, :dim // 2] == 1.0).all() and (out[0, dim // 2:] == 0.0).all()
        assert (out[:1, 0] == 1.0).all() and (out[:1, dim // 2] == 0.0).all()


# ------------------------------------------------------------------------------------------------------------------------- model level
# A tiny UNet whose label MLP has SDXL-base's width (adm_in_channels = 2816: 5 rows per GEMV launch), batch 8 = bench's 4 prompts per call: UNet::set_context
# runs the label MLP as 5 + 3 rows, UNet::run the time MLP and the hoisted lin_embed on 8 -- all of it under the oracle, entry by entry.
T8 = [999, 1, 500, 0, 250, 750, 37, 981]
_model_refs = {}


def _model_case(pkg, dtype):
    ocfg = dataclasses.replace(OC.tiny_config(), adm_in_channels=2816)
    W, _ = weights_for(pkg, ocfg, dtype)
    f16w = dtype in (5, 6, 7)
    x = torch.from_numpy(OC.arb_tensor(8, 4, 16, 16))
    context = torch.from_numpy(OC.arb_tensor(8, 5, ocfg.context_dim))
    y = torch.from_numpy(OC.arb_tensor(8, ocfg.adm_in_channels))
    t = torch.tensor(T8, dtype=torch.int32)
    if f16w not in _model_refs:      # one oracle run per set of weights, shared by the dtypes
        _model_refs[f16w] = OM.unet_forward(ocfg, W, x, t.long(), context, y)
    return ocfg, W, x, t, context, y, _model_refs[f16w]


@pytest.mark.parametrize("dtype", [0, 3, 1, 5])
def test_unet_forward_batch_of_8_with_a_chunked_label_mlp(pkg, ctx, dtype):
    ocfg, W, x, t, context, y, ref = _model_case(pkg, dtype)
    cfg = to_pkg_cfg(pkg, ocfg)
    u = pkg.UNet(ctx, cfg, dtype, weights=pkg.flatten_weights(pkg.unet_param_specs(cfg), {k: v.numpy() for k, v in W.items()}))
    out = u.forward(x.cuda(), t.cuda(), context.cuda(), y.cuda()).cpu()
    per_entry = [rel_err(out[b:b + 1], ref[b:b + 1]) for b in range(8)]
    e = rel_err(out, ref)
    print(f"unet_forward B=8 adm=2816 dtype={dtype}: rel err {e:.3e}; per entry " + " ".join(f"{v:.2e}" for v in per_entry)
          + f"; worst / FWD_TOL {max(per_entry) / FWD_TOL[dtype]:.3f} (entries 0..4 {max(per_entry[:5]):.2e}, 5..7 {max(per_entry[5:]):.2e})")
    if dtype in (0, 3):      # strict modes: every entry against its own reference -- one wrong entry cannot hide behind the others' maximum
        assert all(v < FWD_TOL[dtype] for v in per_entry), per_entry
    else:
        assert e < FWD_TOL[dtype]
    for b in (0, 5, 7):      # both sides of the label MLP's chunk boundary
        alone = u.forward(x[b:b + 1].cuda(), t[b:b + 1].cuda(), context[b:b + 1].cuda(), y[b:b + 1].cuda()).cpu()
        assert torch.equal(alone[0], out[b]), f"entry {b} alone differs from its row in the batch of 8"
