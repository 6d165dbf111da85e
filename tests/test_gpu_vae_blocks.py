"""The autoencoder's attention block and ResnetBlock op by op (sdxl_vae_attn_block / sdxl_vae_res_block: the code Vae::mid and every VAE block run)
against fp64, in the three dtypes a LatentDecoder takes, at the shapes where the chain takes another path: the real width C = 512 in every mode, the
fp32 V^T fallback (HW % 8 != 0), H != W, the un-fused chain in f16 (C = 128), two query passes (8192 + 88 rows, keys padded to 8288); the shortcut
with and without nin_shortcut, one / 12 / 128 row splits of the statistics pass, and batch entries 2^22 apart through the per-entry operand scale.

Bounds come from tests/vae_block_ref.py: margin x the error of the mode's CPU emulation on the same operands, never from a GPU result;
tests/test_cpu_vae_block_ref.py shows that the planted defects (wrong softmax scale, truncated normaliser, dropped pass offset, dropped key tail,
crossed batch entries, P without its lo half or its 2^12, one scale per batch, scale not undone, absmax missing the last row) leave them.

Every assertion prints error / bound first (pytest -s; recorded in profiles/vae_block_tests.txt)."""
import pytest
import torch

import vae_block_ref as R

pytestmark = pytest.mark.gpu

DTYPES = list(R.MODES)      # 0, 1, 3
ATTN_RUNS = [(c[0], dt) for c in R.ATTN_CASES for dt in DTYPES if R.MODES[dt] in R.attn_modes(c[0])]      # (the flat case: f32 and split only)
RES_RUNS = [(c[0], dt) for c in R.RES_CASES for dt in DTYPES if not (c[6] and dt == 1)]      # (an f16 stream cannot hold 2^15 x: the magnitude case runs in f32 and split)


def _dev(d):
    return {k: (None if v is None else v.cuda()) for k, v in d.items()}


def _attn(pkg, ctx, d, dtype, entries=slice(None)):
    """pkg.vae_attn_block on the (device) operands d of a case (entries: a slice of the batch) -> [B,C,H,W] on the device"""
    C = d["x"].shape[1]
    w = lambda k: d["w" + k].reshape(C, C, 1, 1)      # noqa: E731
    return pkg.vae_attn_block(ctx, d["x"][entries].contiguous(), d["gamma"], d["beta"], w("q"), d["bq"], w("k"), d["bk"], w("v"), d["bv"], w("o"), d["bo"],
                              n_group=R.N_GROUP, eps=R.EPS, dtype=dtype)


def _res(pkg, ctx, d, dtype, entries=slice(None)):
    return pkg.vae_res_block(ctx, d["x"][entries].contiguous(), d["gamma1"], d["beta1"], d["w1"], d["b1"], d["gamma2"], d["beta2"], d["w2"], d["b2"],
                             d["w_nin"], d["b_nin"], n_group=R.N_GROUP, eps1=R.EPS, eps2=R.EPS, dtype=dtype)


@pytest.mark.parametrize("name,dtype", ATTN_RUNS)
def test_attn_block_within_emulation_bound(pkg, ctx, name, dtype):
    mode = R.MODES[dtype]
    _, B, C, H, W = R.attn_case(name)
    out = _attn(pkg, ctx, _dev(R.attn_inputs(name)), dtype)
    assert out.shape == (B, C, H, W) and torch.isfinite(out).all()
    rows = torch.from_numpy(R.subset_rows(H * W))
    err = R.attn_error(R._rows(out.cpu())[:, rows], name)
    bound, emu = R.attn_bound(name, mode)
    print(f"vae_attn_block {name} B={B} C={C} {H}x{W} {mode}: error {err:.3e}  bound {bound:.3e} ({R.MARGIN[mode]:g} x emulation {emu:.3e})  ratio {err / bound:.3f}")
    assert err <= bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["base_8x8", "wide_24x40"])
def test_attn_block_entries_are_independent(pkg, ctx, name, dtype):
    d = _dev(R.attn_inputs(name))
    pair, alone = _attn(pkg, ctx, d, dtype), _attn(pkg, ctx, d, dtype, slice(1, 2))
    assert torch.equal(pair[1:2], alone), f"{name} dtype {dtype}: entry 1 alone differs from entry 1 inside the pair by {(pair[1:2] - alone).abs().max().item():.3e}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_attn_block_keeps_no_state_between_launches(pkg, ctx, dtype):
    # the pv_scale scalar and the zero-filled K / V^T buffers are per call: a call at another shape in between changes nothing
    a, b = _dev(R.attn_inputs("wide_24x40")), _dev(R.attn_inputs("ragged_9x9"))
    first = _attn(pkg, ctx, a, dtype)
    assert torch.equal(first, _attn(pkg, ctx, a, dtype))
    other = _attn(pkg, ctx, b, dtype)
    assert torch.equal(first, _attn(pkg, ctx, a, dtype))
    assert torch.equal(other, _attn(pkg, ctx, b, dtype))


@pytest.mark.parametrize("name,dtype", RES_RUNS)
def test_res_block_within_emulation_bound(pkg, ctx, name, dtype):
    mode = R.MODES[dtype]
    _, B, Cin, Cout, H, W, mag = R.res_case(name)
    out = _res(pkg, ctx, _dev(R.res_inputs(name)), dtype)
    assert out.shape == (B, Cout, H, W) and torch.isfinite(out).all()
    errs = R.res_errors(out.cpu(), name)
    bounds, emu = R.res_bounds(name, mode)
    for b in range(B):
        print(f"vae_res_block {name} B={B} {Cin}->{Cout} {H}x{W} {mode} entry {b}: error {errs[b]:.3e}  bound {bounds[b]:.3e} "
              f"({R.MARGIN[mode]:g} x emulation {emu[b]:.3e})  ratio {errs[b] / bounds[b]:.3f}")
    assert all(e <= b for e, b in zip(errs, bounds)), (errs, bounds)


def test_res_block_magnitude_entries_are_independent(pkg, ctx):
    # one operand scale per batch entry: entry 1 (2^-7) next to entry 0 (2^15) gets the bits it gets alone
    d = _dev(R.res_inputs("magnitude_16x24"))
    pair, alone = _res(pkg, ctx, d, 3), _res(pkg, ctx, d, 3, slice(1, 2))
    assert torch.equal(pair[1:2], alone), f"entry 1 alone differs by {(pair[1:2] - alone).abs().max().item():.3e}"


def test_blocks_refuse_bad_arguments(pkg, ctx):
    a, r = _dev(R.attn_inputs("base_8x8")), _dev(R.res_inputs("nin_16x24"))
    C = a["x"].shape[1]
    w = lambda k: a["w" + k].reshape(C, C, 1, 1)      # noqa: E731
    attn = lambda **kw: pkg.vae_attn_block(ctx, *[kw.get(k, v) for k, v in (("x", a["x"]), ("gamma", a["gamma"]), ("beta", a["beta"]), ("wq", w("q")),      # noqa: E731
                                                  ("bq", a["bq"]), ("wk", w("k")), ("bk", a["bk"]), ("wv", w("v")), ("bv", a["bv"]), ("wo", w("o")), ("bo", a["bo"]))],
                                           n_group=kw.get("n_group", R.N_GROUP), eps=R.EPS, dtype=kw.get("dtype", 3))
    res = lambda **kw: pkg.vae_res_block(ctx, *[kw.get(k, r[k]) for k in ("x", "gamma1", "beta1", "w1", "b1", "gamma2", "beta2", "w2", "b2", "w_nin", "b_nin")],      # noqa: E731
                                         n_group=kw.get("n_group", R.N_GROUP), eps1=R.EPS, eps2=R.EPS, dtype=kw.get("dtype", 3))
    for bad in (dict(n_group=0), dict(n_group=7), dict(n_group=512), dict(gamma=None), dict(wq=None), dict(wo=None), dict(dtype=2), dict(dtype=4), dict(dtype=9)):
        with pytest.raises(pkg.EngineError):
            attn(**bad)
    for bad in (dict(n_group=0), dict(n_group=48), dict(gamma1=None), dict(w2=None), dict(dtype=2), dict(dtype=5), dict(w_nin=None, b_nin=None), dict(w_nin=None)):
        with pytest.raises(pkg.EngineError):
            res(**bad)
    # the context stays usable, and biases are optional
    assert torch.isfinite(attn(bq=None, bo=None)).all() and torch.isfinite(res(b1=None, b_nin=None)).all()
