"""One CLIP encoder layer and the pooled head op by op against fp64, through the model's own code (ClipText::block / ClipText::run of csrc/clip.cpp), at
the widths a real prompt runs -- 768 / 12 heads / QuickGELU and 1280 / 20 heads / GELU(erf), where the GEMM selection picks other tiles and families than
at the 128 / 192 of test_gpu_clip.py -- in the three dtypes a CLIP takes.  A one-layer tower whose token table holds the case's input rows IS the single
layer (hidden_idx 0: the embedding, 1: the stream after the layer, forward_hidden_pooled: the head); the second call of a shape runs the captured graph.

What the cases reach: the fused Q|K|V projection's transposed V^T store with 77 rows per entry (every row tile straddles batch entries; M = 231 is
odd), the in-place residual epilogues on an f16 and an fp32 stream, the GELU / QuickGELU epilogues, masked d = 64 attention at 77 keys padded to 128,
at 64 keys without the V^T zero fill, at 9 and at 1 key, embed_tokens / argmax_rows / gather_rows, the LayerNorm of the selected rows, the bias-free
text_projection GEMV in chunks of 8 + 1, and the per-shape graph capture.

Bounds come from tests/clip_layer_ref.py: margin x the error of the mode's CPU emulation on the same operands, never from a GPU result;
tests/test_cpu_clip_layer_ref.py shows that the planted defects (mask shifted / off, a 4-key V^T group in its first row's entry, the key tail in the
normaliser, heads rotated, scale C^-1/2, activations swapped, residual taken from the LayerNorm output or dropped, position by flat row, last / next EOT
row, pooled without LayerNorm) leave them.

Every bound assertion prints error / bound first (pytest -s; recorded in profiles/clip_layer_tests.txt)."""
import pytest
import torch

import clip_layer_ref as R

pytestmark = pytest.mark.gpu

DTYPES = list(R.MODES)      # 0, 1, 2
WIDTHS = list(R.WIDTHS)
LAYER_RUNS = [(n, w, dt, "full") for n in R.LAYER_CASES for w in WIDTHS for dt in DTYPES] + \
             [(n, w, dt, ws) for ws in ("attn_only", "mlp_only") for n in ("pair_77", "short_9") for w in WIDTHS for dt in DTYPES]
POOL_RUNS = [(n, w, dt) for n in R.POOL_CASES for w in R.case(n)[4] for dt in DTYPES]

_models = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _models.clear()


def _build(pkg, ctx, name, width, wset, dtype, n_layer=1):
    _, B, S, _, _, _ = R.case(name)
    H, quick = R.WIDTHS[width]
    cfg = pkg.CLIPConfig(B * S, width, R.embed_dim(name, width), H, R.N_CTX, n_layer, quick)
    flat = pkg.flatten_weights(pkg.clip_param_specs(cfg), R.model_weights(name, width, wset, n_layer))
    return pkg.CLIP(ctx, cfg, dtype, weights=flat)


def _model(pkg, ctx, name, width, wset, dtype, n_layer=1):
    """the tower on the case's token table: built once per (case, width, weight set, dtype) for the module"""
    key = (name, width, wset, dtype, n_layer)
    if key not in _models:
        _models[key] = _build(pkg, ctx, name, width, wset, dtype, n_layer)
    return _models[key]


def _ids(name, width):
    return R.case_inputs(name, width)["ids"]


def _report(tag, errs, bounds, emu, margin):
    for b, (e, bd, em) in enumerate(zip(errs, bounds, emu)):
        print(f"{tag} entry {b}: error {e:.3e}  bound {bd:.3e} ({margin:g} x emulation {em:.3e})  ratio {e / bd:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", WIDTHS)
def test_embedding_bit_for_bit(pkg, ctx, width, dtype):
    name = R.EMBED_CASE[0]
    c = R.case_inputs(name, width)
    ids = c["ids"]
    assert ids.shape == (3, 9) and int(ids.min()) == 0 and int(ids.max()) == 26 and len(set(ids.flatten().tolist())) < 27 and R.N_CTX == 77
    out = _model(pkg, ctx, name, width, "full", dtype).forward_hidden(ids, 0).cpu()
    want = R.embed_expected(c["tok"], c["pos"], ids, R.MODES[dtype])
    assert torch.equal(out, want), f"{(out != want).sum().item()} of {out.numel()} elements differ, by {(out - want).abs().max().item():.3e} at most"


@pytest.mark.parametrize("name,width,dtype,wset", LAYER_RUNS)
def test_layer_within_emulation_bound(pkg, ctx, name, width, dtype, wset):
    mode = R.MODES[dtype]
    _, B, S, _, _, _ = R.case(name)
    m, ids = _model(pkg, ctx, name, width, wset, dtype), _ids(name, width)
    out = m.forward_hidden(ids, 1).cpu()
    assert out.shape == (B, S, width) and torch.isfinite(out).all()
    errs = R.layer_errors(out, name, width, wset)
    bounds, emu = R.layer_bounds(name, width, wset, mode)
    _report(f"clip_layer {name} B={B} S={S} C={width} {wset} {mode}", errs, bounds, emu, R.MARGIN[mode])
    assert all(e <= b for e, b in zip(errs, bounds)), (errs, bounds)
    assert torch.equal(m.forward_hidden(ids, 1).cpu(), out), "the next call of the shape (captured / replayed) differs from this one"
    assert torch.equal(m.forward_hidden(ids, 0).cpu(), R.embed_expected(*(R.case_inputs(name, width)[k] for k in ("tok", "pos", "ids")), mode))


@pytest.mark.parametrize("name,width,dtype", POOL_RUNS)
def test_pooled_head_within_bound(pkg, ctx, name, width, dtype):
    mode = R.MODES[dtype]
    _, B, S, _, _, wset = R.case(name)
    m, ids = _model(pkg, ctx, name, width, wset, dtype), _ids(name, width)
    hidden, pooled = m.forward_hidden_pooled(ids, 0)
    hidden, pooled = hidden.cpu(), pooled.cpu()
    assert pooled.shape == (B, R.embed_dim(name, width)) and torch.isfinite(pooled).all()
    errs = R.pooled_errors(pooled, name, width, wset)
    bounds, emu = R.pooled_bounds(name, width, wset, mode)
    _report(f"clip_pooled {name} B={B} S={S} C={width} E={pooled.shape[1]} {mode}", errs, bounds, emu, R.MARGIN[mode])
    assert all(e <= b for e, b in zip(errs, bounds)), (errs, bounds)
    # the tap beside it is what forward_hidden returns; with both branches knocked out the layer hands the embedding on bit for bit
    assert torch.equal(hidden, m.forward_hidden(ids, 0).cpu())
    assert torch.equal(m.forward_hidden(ids, 1).cpu(), hidden)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", WIDTHS)
def test_entries_are_independent_at_real_width(pkg, ctx, width, dtype):
    m, ids = _model(pkg, ctx, "odd_77", width, "full", dtype), _ids("odd_77", width)
    batch, alone = m.forward_hidden(ids, 1), m.forward_hidden(ids[1:2], 1)
    assert torch.equal(batch[1:2], alone), f"entry 1 alone differs from entry 1 inside the batch by {(batch[1:2] - alone).abs().max().item():.3e}"
    m, ids = _model(pkg, ctx, "pool_9x77", width, "head", dtype), _ids("pool_9x77", width)
    batch, alone = m.forward_hidden_pooled(ids, 0)[1], m.forward_hidden_pooled(ids[8:9], 0)[1]
    assert torch.equal(batch[8:9], alone), f"pooled entry 8 alone differs from entry 8 inside the batch by {(batch[8:9] - alone).abs().max().item():.3e}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", WIDTHS)
def test_layer_is_causal_at_real_width(pkg, ctx, width, dtype):
    m, ids = _model(pkg, ctx, "pair_77", width, "full", dtype), _ids("pair_77", width)
    other = ids.clone()
    other[0, 40] = ids[1, 5]
    assert int(other[0, 40]) != int(ids[0, 40])
    a, b = m.forward_hidden(ids, 1), m.forward_hidden(other, 1)
    assert torch.equal(a[0, :40], b[0, :40]), f"rows before the replaced token moved by {(a[0, :40] - b[0, :40]).abs().max().item():.3e}"
    assert bool((a[0, 40:] != b[0, 40:]).any(-1).all()), "a row at or after the replaced token did not change"
    assert torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", WIDTHS)
def test_replay_keeps_no_state(pkg, ctx, width, dtype):
    # a model of its own, so that the calls are the eager one, the capture and a replay; short_9's ids index the same table
    m = _build(pkg, ctx, "pair_77", width, "full", dtype)
    ids, short = _ids("pair_77", width), _ids("short_9", width)
    runs = [m.forward_hidden(ids, 1).clone() for _ in range(3)]
    mid = m.forward_hidden(short, 1).clone()
    runs += [m.forward_hidden(ids, 1).clone() for _ in range(2)]
    assert all(torch.equal(runs[0], r) for r in runs[1:]), [float((runs[0] - r).abs().max()) for r in runs[1:]]
    assert torch.equal(mid, m.forward_hidden(short, 1))
    # the key holds hidden / pooled / tap: the pooled pass and the hidden pass take turns on one model
    h0, p0 = (t.clone() for t in m.forward_hidden_pooled(ids, 0))
    assert torch.equal(m.forward_hidden(ids, 1), runs[0])
    h1, p1 = (t.clone() for t in m.forward_hidden_pooled(ids, 0))
    assert torch.equal(m.forward_hidden(ids, 0), h0)
    h2, p2 = m.forward_hidden_pooled(ids, 0)
    assert torch.equal(h0, h1) and torch.equal(h0, h2) and torch.equal(p0, p1) and torch.equal(p0, p2)
    assert torch.equal(m.forward_hidden(ids, 1), runs[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_tap_of_a_two_layer_tower(pkg, ctx, dtype):
    ids = _ids("pair_77", 768)
    one, two = _model(pkg, ctx, "pair_77", 768, "full", dtype), _model(pkg, ctx, "pair_77", 768, "full", dtype, n_layer=2)
    first = one.forward_hidden(ids, 1)
    assert torch.equal(two.forward_hidden(ids, 1), first)
    assert torch.equal(two.forward_hidden_pooled(ids, 1)[0], first)
    last = two.forward_hidden(ids, 2)
    assert torch.isfinite(last).all() and bool((last != first).any(-1).all())
    assert torch.equal(two.forward_hidden(ids, 0), one.forward_hidden(ids, 0))
