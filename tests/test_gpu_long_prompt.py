"""Embedder.tokens_to_conditioning on a prompt of several 77-token chunks (ids [c, 77]): every chunk is encoded as a batch row of its own, the hidden
states are concatenated along the token axis to [1, 77 c, .], the pooled embedding is chunk 0's.  Against oracle/clip.py run chunk by chunk and
concatenated, at the tolerances of tests/test_gpu_clip.py; ids [1, 77] keep the bits they had (checked against a direct forward_hidden call)."""
import pytest
import torch

from oracle import clip as OCL, config as OC, model as OM
from test_gpu_clip import TOL, _ids, _pcfg
from util import rel_err

pytestmark = pytest.mark.gpu

SIZE, CROP, AR = torch.tensor([[1024, 1024]]), torch.tensor([[0, 0]]), torch.tensor([1024, 1024])


def _embedders(pkg, ctx, dtype):
    c1, c2 = OCL.tiny_clip_config(), OCL.tiny_open_clip_config()
    W1, W2 = (OM.to_torch(OC.synth_weights(OCL.clip_param_specs(c), s)) for c, s in ((c1, 1), (c2, 2)))
    m1, m2 = pkg.CLIP(ctx, _pcfg(pkg, c1), dtype, seed=1), pkg.CLIP(ctx, _pcfg(pkg, c2), dtype, seed=2)
    return (c1, W1, m1), (c2, W2, m2), pkg.Embedder(ctx, m1, m2)


@pytest.mark.parametrize("dtype", [0, 1])
def test_three_chunks_against_the_oracle_chunk_by_chunk(pkg, ctx, dtype):
    (c1, W1, _), (c2, W2, _), e = _embedders(pkg, ctx, dtype)
    ids_c, ids_o = _ids(3, 77, 5, 49407, eot_at=[76, 76, 20]), _ids(3, 77, 5, 0, eot_at=[76, 76, 20])
    un_c, un_o = _ids(3, 77, 6, 49407, eot_at=[30, 1, 1]), _ids(3, 77, 6, 0, eot_at=[30, 1, 1])
    got = e.tokens_to_conditioning(ids_c, ids_o, un_c, un_o, SIZE, CROP, AR)
    oe = OCL.Embedder(c1, W1, c2, W2)
    per_chunk = [oe.tokens_to_conditioning(ids_c[i:i + 1], ids_o[i:i + 1], un_c[i:i + 1], un_o[i:i + 1], SIZE, CROP, AR) for i in range(3)]
    for name in ("context_full", "context_open_clip", "unconditional_context_full", "unconditional_context_open_clip"):
        ref = torch.cat([getattr(p, name) for p in per_chunk], dim=-2)      # along the token axis
        a = getattr(got, name)
        assert tuple(a.shape) == tuple(ref.shape) and a.shape[-2] == 231, name
        assert rel_err(a, ref) < TOL[dtype], (name, rel_err(a, ref))
    for name in ("channel_context", "channel_context_refiner", "unconditional_channel_context", "unconditional_channel_context_refiner"):
        a, ref = getattr(got, name), getattr(per_chunk[0], name)               # pooled: chunk 0's
        assert tuple(a.shape) == tuple(ref.shape), name
        assert rel_err(a, ref) < TOL[dtype], (name, rel_err(a, ref))
    # ... and exactly chunk 0's: the label vectors of the first chunk encoded alone
    first = e.tokens_to_conditioning(ids_c[:1], ids_o[:1], un_c[:1], un_o[:1], SIZE, CROP, AR)
    assert torch.equal(got.channel_context, first.channel_context) and torch.equal(got.unconditional_channel_context, first.unconditional_channel_context)
    assert torch.equal(got.context_full[:, :77], first.context_full)           # batch rows are independent: a chunk has the bits it has alone


def test_one_chunk_keeps_its_bits(pkg, ctx):
    (c1, _, m1), (c2, _, m2), e = _embedders(pkg, ctx, 1)
    ids_c, ids_o = _ids(1, 77, 5, 49407, eot_at=[9]), _ids(1, 77, 5, 0, eot_at=[9])
    un_c, un_o = _ids(1, 77, 6, 49407, eot_at=[1]), _ids(1, 77, 6, 0, eot_at=[1])
    got = e.tokens_to_conditioning(ids_c, ids_o, un_c, un_o, SIZE, CROP, AR)
    h1 = m1.forward_hidden(torch.cat([un_c, ids_c]), c1.n_layer - 1)
    h2, _ = m2.forward_hidden_pooled(torch.cat([un_o, ids_o]), c2.n_layer - 1)
    full = torch.cat([h1, h2], dim=2)
    assert torch.equal(got.context_full, full[1:2]) and torch.equal(got.unconditional_context_full, full[0])
    assert torch.equal(got.context_open_clip, h2[1:2]) and torch.equal(got.unconditional_context_open_clip, h2[0])


def test_chunk_counts_must_agree(pkg, ctx):
    _, _, e = _embedders(pkg, ctx, 1)
    two, one = _ids(2, 77, 5, 0), _ids(1, 77, 5, 0)
    with pytest.raises(ValueError):
        e.tokens_to_conditioning(two, two, one, one, SIZE, CROP, AR)
    with pytest.raises(ValueError):
        e.tokens_to_conditioning(*([_ids(5, 77, 5, 0)] * 4), SIZE, CROP, AR)
