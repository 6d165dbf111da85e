"""The fused query projection + cross-attention of the f16 engine on the weights-in-registers GEMM (csrc/igemm_wreg.hip, XA instantiation).

Everything goes through pkg.ln_query_cross_attention(..., fused=True) against the reference of test_gpu_ops.test_ln_query_cross_attention
(OM.layer_norm(x) @ wq -> OM.qkv_attention, one dominant key, the f16 bound TOL[1] of that file).  The tile height is forced through the
"igemm_variant" knob (60 = 96 rows, 62 = 64 rows per tile), the kernel family through "wreg_xattn" (0 = the pipe kernels' epilogue form).
"""
import math

import pytest
import torch

from oracle import model as OM
from util import rel_err, seeded

pytestmark = pytest.mark.gpu

TOL_F16 = 4e-3          # TOL[1] of tests/test_gpu_ops.py: one f16 rounding of the operands plus the f16 rounding of the stored result

_CASES = {}


def _case(B, Nq, Nk, C, seed=21):
    """inputs and the fp32 oracle result of one shape, computed once per session"""
    key = (B, Nq, Nk, C, seed)
    if key not in _CASES:
        x = (seeded(B, Nq, C, seed=seed) * 1.5 + 0.2).half().float()
        gamma, beta = 1 + 0.1 * seeded(C, seed=5), 0.1 * seeded(C, seed=6)
        wq = seeded(C, C, seed=seed + 1) / math.sqrt(C)
        k, v = seeded(B, Nk, C, seed=seed + 2), seeded(B, Nk, C, seed=seed + 3)
        k[0, 0] *= 3.0                                   # one dominant key: the softmax is not near-uniform
        q = OM.layer_norm(x, gamma, beta, 1e-5) @ wq
        ref = OM.qkv_attention(q, k, v, None, C // 64)
        _CASES[key] = (tuple(t.cuda() for t in (x, gamma, beta, wq, k, v)), ref)
    return _CASES[key]


def _run(pkg, ctx, dev, fused=True, entry=None):
    x, gamma, beta, wq, k, v = dev
    if entry is not None:
        x, k, v = x[entry:entry + 1].contiguous(), k[entry:entry + 1].contiguous(), v[entry:entry + 1].contiguous()
    return pkg.ln_query_cross_attention(ctx, x, gamma, beta, wq, k, v, 1e-5, fused)


class _Knobs:
    """igemm_variant / wreg_xattn for the duration of a block; both restored whatever happens inside"""

    def __init__(self, pkg, variant=0, wreg_xattn=1):
        self.pkg, self.variant, self.wreg_xattn = pkg, variant, wreg_xattn

    def __enter__(self):
        self.pkg.debug_set("igemm_variant", self.variant)
        self.pkg.debug_set("wreg_xattn", self.wreg_xattn)
        return self

    def set(self, variant=None, wreg_xattn=None):
        if variant is not None:
            self.pkg.debug_set("igemm_variant", variant)
        if wreg_xattn is not None:
            self.pkg.debug_set("wreg_xattn", wreg_xattn)

    def __exit__(self, *exc):
        try:
            self.pkg.debug_set("igemm_variant", 0)
        finally:
            self.pkg.debug_set("wreg_xattn", 1)
        return False


# (2, 64, 77, 128) at 96 rows: tile 0 straddles both entries, two heads, two k-tiles (one per k-group: fewer than the prefetch depth), a 32-row tail
# tile; (1, 128, 96, 128): the maximum key count; (3, 64, 5, 256): few keys (masking), three entries in two 96-row tiles; (2, 256, 33, 1280): the
# production width; the last two: the step's own launches at the 32^2 / 64^2 levels, once each with the automatic tile height.
@pytest.mark.parametrize("B,Nq,Nk,C,variant", [
    (2, 64, 77, 128, 60), (2, 64, 77, 128, 62),
    (1, 128, 96, 128, 60), (1, 128, 96, 128, 62),
    (3, 64, 5, 256, 60), (3, 64, 5, 256, 62),
    (2, 256, 33, 1280, 60), (2, 256, 33, 1280, 62),
    (2, 1024, 77, 1280, 0), (1, 4096, 77, 640, 0),
])
def test_wreg_xattn_against_the_oracle(pkg, ctx, B, Nq, Nk, C, variant):
    dev, ref = _case(B, Nq, Nk, C)
    with _Knobs(pkg, variant, 1) as kn:
        out = _run(pkg, ctx, dev)
        kn.set(variant=0, wreg_xattn=0)
        pipe = _run(pkg, ctx, dev)
    e, ep = rel_err(out, ref), rel_err(pipe, ref)
    print(f"wreg_xattn B={B} Nq={Nq} Nk={Nk} C={C} variant={variant}: rel err {e:.3e} (pipe form {ep:.3e}); "
          f"{float((out != pipe).float().mean()):.2e} of the outputs differ between the two forms")
    assert e < TOL_F16


@pytest.mark.parametrize("B,Nq,Nk,C", [(2, 64, 77, 128), (2, 256, 33, 1280)])
@pytest.mark.parametrize("variant", [0, 60])
def test_wreg_xattn_entry_does_not_depend_on_its_batch(pkg, ctx, B, Nq, Nk, C, variant):
    dev, _ = _case(B, Nq, Nk, C)
    with _Knobs(pkg, variant, 1):
        batched = _run(pkg, ctx, dev)
        for b in range(B):
            alone = _run(pkg, ctx, dev, entry=b)
            assert torch.equal(alone[0], batched[b]), f"entry {b} differs alone / batched (variant {variant})"


@pytest.mark.parametrize("B,Nq,Nk,C,variant", [(2, 64, 77, 128, 60), (3, 64, 5, 256, 62), (2, 256, 33, 1280, 60), (2, 256, 33, 1280, 62)])
def test_wreg_xattn_keeps_nothing_between_launches(pkg, ctx, B, Nq, Nk, C, variant):
    # two input sets alternating over four launches: a q fragment read before the hand-over rendezvous, or a K fragment left from the launch before,
    # would make a repeat differ from the first result of its set
    sets = [_case(B, Nq, Nk, C)[0], _case(B, Nq, Nk, C, seed=41)[0]]
    with _Knobs(pkg, variant, 1):
        first = [None, None]
        for launch in range(4):
            o = _run(pkg, ctx, sets[launch & 1])
            if first[launch & 1] is None:
                first[launch & 1] = o
            else:
                assert torch.equal(o, first[launch & 1]), f"launch {launch} differs from the first result of its input set"
    assert not torch.equal(first[0], first[1])


@pytest.mark.parametrize("B,Nq,Nk,C", [(3, 192, 5, 192), (1, 128, 96, 64)])
def test_wreg_xattn_widths_off_the_tile_stay_on_the_pipe_kernels(pkg, ctx, B, Nq, Nk, C):
    # N is no multiple of 128: no weights-in-registers form -- the launch keeps the pipe kernels' epilogue and its result
    dev, ref = _case(B, Nq, Nk, C)
    with _Knobs(pkg, 0, 1) as kn:
        on = _run(pkg, ctx, dev)
        kn.set(wreg_xattn=0)
        off = _run(pkg, ctx, dev)
    e = rel_err(on, ref)
    print(f"wreg_xattn fallback B={B} Nq={Nq} Nk={Nk} C={C}: rel err {e:.3e}")
    assert e < TOL_F16
    assert torch.equal(on, off)


@pytest.mark.parametrize("B,Nq,Nk,C", [(2, 64, 77, 128), (2, 256, 33, 1280)])
def test_wreg_xattn_leaves_the_split_precision_form_alone(pkg, ctx, B, Nq, Nk, C):
    dev, _ = _case(B, Nq, Nk, C)
    with _Knobs(pkg, 0, 1) as kn:
        on = _run(pkg, ctx, dev, fused=2)
        kn.set(wreg_xattn=0)
        off = _run(pkg, ctx, dev, fused=2)
    assert torch.equal(on, off)
