"""The fused query projection + cross-attention over a LONG context (97 .. 384 keys: two to four 77-token chunks of a prompt) on the
weights-in-registers GEMM: csrc/igemm_wreg.hip, XA = 2 instantiation, csrc/igemm_common.h xattn_unit_long (96-key blocks, online softmax).

The pattern of tests/test_gpu_wreg_xattn.py: pkg.ln_query_cross_attention(..., fused=True) against OM.layer_norm(x) @ wq -> OM.qkv_attention inside
the f16 bound TOL_F16; the error of the un-fused pair (projection + attention kernel) on the same inputs is printed beside it.  Shapes, inputs and
what each exercises: tests/xattn_long_ref.py (the CPU test shows there that the clean arithmetic stays below half the bound on these inputs and that a
skipped rescale, a mask without the block offset, a dropped last block and an un-rescaled row sum land at least ten times outside it).

Widths that are no multiple of 128 have no weights-in-registers form: above 96 keys fused=True is REFUSED for them (never run un-fused silently);
fused=2 (split precision) keeps its 96-key limit; more than 384 keys are refused.
"""
import pytest
import torch

import xattn_long_ref as XR
from oracle import model as OM
from util import rel_err

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(B, Nq, Nk, C, **kw):
    """inputs on the device and the fp32 oracle result of one case, computed once per session"""
    key = (B, Nq, Nk, C, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _CASES:
        x, gamma, beta, wq, k, v = XR.inputs(B, Nq, Nk, C, **kw)
        ref = OM.qkv_attention(OM.layer_norm(x, gamma, beta, 1e-5) @ wq, k, v, None, C // 64)
        _CASES[key] = (tuple(t.cuda() for t in (x, gamma, beta, wq, k, v)), ref)
    return _CASES[key]


def _run(pkg, ctx, dev, fused=True, entry=None):
    x, gamma, beta, wq, k, v = dev
    if entry is not None:
        x, k, v = x[entry:entry + 1].contiguous(), k[entry:entry + 1].contiguous(), v[entry:entry + 1].contiguous()
    return pkg.ln_query_cross_attention(ctx, x, gamma, beta, wq, k, v, 1e-5, fused)


class _Variant:
    """the forced tile height ("igemm_variant": 60 = 96 rows, 62 = 64 rows per tile) for the duration of a block"""

    def __init__(self, pkg, variant):
        self.pkg, self.variant = pkg, variant

    def __enter__(self):
        self.pkg.debug_set("igemm_variant", self.variant)
        return self

    def __exit__(self, *exc):
        self.pkg.debug_set("igemm_variant", 0)
        return False


@pytest.mark.parametrize("index", range(len(XR.SHAPES)), ids=["%dx%dx%dx%d-v%d" % s for s in XR.SHAPES])
def test_long_xattn_against_the_oracle(pkg, ctx, index):
    B, Nq, Nk, C, variant = XR.SHAPES[index]
    dev, ref = _case(B, Nq, Nk, C, rot=index)
    with _Variant(pkg, variant):
        out = _run(pkg, ctx, dev)
    unfused = _run(pkg, ctx, dev, fused=False)
    e, eu = rel_err(out, ref), rel_err(unfused, ref)
    print(f"long xattn B={B} Nq={Nq} Nk={Nk} C={C} variant={variant}: rel err {e:.3e} (un-fused pair {eu:.3e})")
    assert torch.isfinite(out).all()
    assert e < XR.TOL_F16


def test_long_xattn_weights_of_earlier_blocks_may_underflow(pkg, ctx):
    B, Nq, Nk, C, variant = XR.UNDERFLOW
    dev, ref = _case(B, Nq, Nk, C, kinds=["last"] * B, factor=8.0)
    with _Variant(pkg, variant):
        out = _run(pkg, ctx, dev)
    unfused = _run(pkg, ctx, dev, fused=False)
    e, eu = rel_err(out, ref), rel_err(unfused, ref)
    print(f"long xattn x8 key in the last block B={B} Nq={Nq} Nk={Nk} C={C}: rel err {e:.3e} (un-fused pair {eu:.3e})")
    assert torch.isfinite(out).all()
    assert e < XR.TOL_F16


@pytest.mark.parametrize("index", [0, 2, 6, 8])
def test_long_xattn_entry_does_not_depend_on_its_batch(pkg, ctx, index):
    B, Nq, Nk, C, variant = XR.SHAPES[index]
    dev, _ = _case(B, Nq, Nk, C, rot=index)
    with _Variant(pkg, variant):
        batched = _run(pkg, ctx, dev)
        for b in range(B):
            alone = _run(pkg, ctx, dev, entry=b)
            assert torch.equal(alone[0], batched[b]), f"entry {b} differs alone / batched"


@pytest.mark.parametrize("index", [1, 2, 6])
def test_long_xattn_keeps_nothing_between_launches(pkg, ctx, index):
    # two input sets alternating over four launches: a K / V^T block left in registers or a stale running maximum would make a repeat differ
    B, Nq, Nk, C, variant = XR.SHAPES[index]
    sets = [_case(B, Nq, Nk, C, rot=index)[0], _case(B, Nq, Nk, C, rot=index + 1, seed=41)[0]]
    with _Variant(pkg, variant):
        first = [None, None]
        for launch in range(4):
            o = _run(pkg, ctx, sets[launch & 1])
            if first[launch & 1] is None:
                first[launch & 1] = o
            else:
                assert torch.equal(o, first[launch & 1]), f"launch {launch} differs from the first result of its input set"
    assert not torch.equal(first[0], first[1])


def test_more_than_384_keys_are_refused(pkg, ctx):
    dev, _ = _case(1, 64, 385, 128)
    with pytest.raises(pkg.EngineError, match="fused cross-attention: unsupported shape"):
        _run(pkg, ctx, dev)
    B, Nq, Nk, C, _ = XR.SHAPES[2]
    dev, ref = _case(B, Nq, Nk, C, rot=2)
    assert rel_err(_run(pkg, ctx, dev), ref) < XR.TOL_F16      # the next valid call works


def test_split_precision_form_keeps_its_96_keys(pkg, ctx):
    B, Nq, Nk, C, _ = XR.SHAPES[2]
    dev, _ = _case(B, Nq, Nk, C, rot=2)
    with pytest.raises(pkg.EngineError, match="fused cross-attention: unsupported shape"):
        _run(pkg, ctx, dev, fused=2)


@pytest.mark.parametrize("C", [192, 64])
def test_widths_off_the_tile_are_refused_above_96_keys(pkg, ctx, C):
    dev, ref = _case(2, 64, 154, C)
    with pytest.raises(pkg.EngineError, match="fused cross-attention: unsupported shape"):
        _run(pkg, ctx, dev)
    assert rel_err(_run(pkg, ctx, dev, fused=False), ref) < XR.TOL_F16
