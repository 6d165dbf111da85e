"""The per-step, per-entry ControlNet add (sdxl_skip_residual_add_steps) on the GPU against fp64: entry boundaries inside a wave and a workgroup, more
chunks than one trip of the grid, the row of the scale table the device step index names, entries at scale 0 whose sources hold NaN, cond_only
through the op, refusals that write nothing."""
import numpy as np
import pytest
import torch

from skip_add_ref import skip_add_expected
from util import rounding_slack, seeded

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _spacing32(v):
    """spacing of the fp32 numbers at |v|"""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23.0)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------- 1. the add op
# (rows per entry, C, ld, col_off): one row per entry (entries change inside a wave); 37 rows of 8 / 16 chunks (the boundary at chunk 296 / 592 lies
# inside a wave and inside a workgroup); more chunks than the capped grid covers in one trip (2048 x 256), a small segment behind it
OP_SEGS = [(1, 8, 8, 0), (37, 64, 192, 128), (8209, 320, 320, 0), (3, 8, 24, 8)]
# row 1 is never named by the step index: NaN there shows that the kernel reads the row it is told to
OP_TABLES = {2: [[1.0, -0.37] + [NAN] * 6, [NAN] * 8, [0.0, 1.0] + [NAN] * 6],
             3: [[1.0, -0.37, 0.0] + [NAN] * 5, [NAN] * 8, [-0.37, 0.0, 1.0] + [NAN] * 5]}


@pytest.mark.parametrize("step", [0, 2], ids=["first", "last"])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("tdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_step_add_op_against_fp64(pkg, ctx, tdt, B, step):
    scales = OP_TABLES[B][step][:B]
    bufs = [seeded(B * r, ld, seed=100 + i).to(tdt) for i, (r, C, ld, off) in enumerate(OP_SEGS)]
    srcs = [seeded(B * r, C, seed=200 + i).to(tdt) for i, (r, C, ld, off) in enumerate(OP_SEGS)]
    for (r, C, ld, off), s in zip(OP_SEGS, srcs):      # the sources of an entry at scale 0 hold NaN: they must not be read into the sum
        for b in range(B):
            if scales[b] == 0.0:
                s[b * r:(b + 1) * r] = NAN
    table = torch.tensor(OP_TABLES[B], dtype=torch.float32).cuda()

    def run(step_idx):
        d = [b.cuda() for b in bufs]
        s = [x.cuda() for x in srcs]
        pkg.skip_residual_add_steps(ctx, [(b[:, off:off + C], x) for b, x, (_, C, _, off) in zip(d, s, OP_SEGS)], B, table, step_idx)
        return [b.cpu() for b in d]

    outs, again = run(step), run(torch.tensor([step], dtype=torch.int32, device="cuda"))
    worst = 0.0
    for out, rep, buf, src, (r, C, ld, off) in zip(outs, again, bufs, srcs, OP_SEGS):
        assert torch.equal(_bits(out), _bits(rep)), "two runs differ"
        keep = torch.ones(ld, dtype=torch.bool)
        keep[off:off + C] = False
        assert torch.equal(_bits(out[:, keep]), _bits(buf[:, keep])), "columns outside the slice changed"
        for b in range(B):
            rows = slice(b * r, (b + 1) * r)
            got, old = out[rows, off:off + C], buf[rows, off:off + C]
            if scales[b] == 0.0:
                assert torch.equal(_bits(got), _bits(old)), f"entry {b} at scale 0 changed (its source is NaN)"
                continue
            ref = old.double() + float(np.float32(scales[b])) * src[rows].double()      # (exact in fp64; the kernel rounds the exact sum once to fp32)
            if tdt == torch.float32:
                bound, err = 0.5 * _spacing32(ref) * (1 + 2.0 ** -20), (got.double() - ref).abs()
            else:      # one more rounding, fp32 -> f16: f16(ref), or its neighbour where the fp32 value may sit across a rounding midpoint
                h, bound = rounding_slack(ref, 0.5 * _spacing32(ref))
                err = (got.double() - h).abs()
            assert bool((err <= bound).all()), f"segment {(r, C, ld, off)} entry {b}: max err {err.max():.3e}"
            assert not torch.equal(got, old)
            worst = max(worst, (got.double() - ref).abs().max().item())
            want = torch.from_numpy(skip_add_expected(old.numpy(), [src[rows].numpy()], [scales[b]], old.numpy().dtype))
            differ = int((_bits(got) != _bits(want)).sum())
            print(f"segment {(r, C, ld, off)} entry {b}: {differ} of {want.numel()} elements differ from the expected bits")
            assert differ == 0
    print(f"skip_residual_add_steps B {B} {tdt} step {step} scales {scales}: max |out - fp64| {worst:.3e}")


def test_step_add_op_cond_only_is_the_second_half_at_zero(pkg, ctx):
    """cond_only is per-entry scales with the pair's second half at 0: the add under such a row leaves the unconditional entries' bits alone (their
    sources hold NaN) and gives the conditional ones what the one-scalar entry gives them"""
    n, r, C = 2, 37, 64
    tab = np.zeros((5, 8), dtype=np.float32)
    tab[:4, 0], tab[:4, 1] = 1.0, -0.37
    buf, src = seeded(2 * n * r, C, seed=7).half(), seeded(2 * n * r, C, seed=8).half()
    src[n * r:] = NAN
    d = buf.cuda()
    pkg.skip_residual_add_steps(ctx, [(d, src.cuda())], 2 * n, torch.from_numpy(tab).cuda(), 3)
    assert torch.equal(_bits(d[n * r:].cpu()), _bits(buf[n * r:]))
    for b, s in enumerate((1.0, -0.37)):
        one = buf[b * r:(b + 1) * r].cuda()
        pkg.skip_residual_add(ctx, [(one, src[b * r:(b + 1) * r].cuda())], s)
        assert torch.equal(_bits(d[b * r:(b + 1) * r].cpu()), _bits(one.cpu()))


@pytest.mark.parametrize("tdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_step_add_op_one_scale_for_every_entry_is_the_one_scalar_add(pkg, ctx, tdt):
    """a table row whose B entries hold the same non-zero scale gives the bits of the one-scalar entry at that scale"""
    B, (r, C, ld, off) = 3, OP_SEGS[1]
    buf, src = seeded(B * r, ld, seed=21).to(tdt), seeded(B * r, C, seed=22).to(tdt)
    table = torch.tensor([[NAN] * 8, [-0.37] * B + [NAN] * (8 - B)], dtype=torch.float32).cuda()
    steps, one = buf.cuda(), buf.cuda()
    pkg.skip_residual_add_steps(ctx, [(steps[:, off:off + C], src.cuda())], B, table, 1)
    pkg.skip_residual_add(ctx, [(one[:, off:off + C], src.cuda())], -0.37)
    assert torch.equal(_bits(steps.cpu()), _bits(one.cpu()))
    assert not torch.equal(_bits(steps.cpu()), _bits(buf))


def test_step_add_op_refusals_write_nothing(pkg, ctx):
    buf, src = seeded(6, 64, seed=1), seeded(6, 64, seed=2)
    table = torch.ones(2, 8, device="cuda")
    for B, word in ((4, "multiple of B"), (0, "1..8"), (9, "1..8")):
        d = buf.cuda()
        with pytest.raises(pkg.InvalidArgument, match=word):
            pkg.skip_residual_add_steps(ctx, [(d, src.cuda())], B, table, 0)
        assert torch.equal(d.cpu(), buf)
    d = buf.cuda()
    with pytest.raises(pkg.InvalidArgument):      # what the one-scalar entry refuses: a slice off a 16-byte boundary
        pkg.skip_residual_add_steps(ctx, [(d[:, 1:9], src[:, :8].contiguous().cuda())], 2, table, 0)
    with pytest.raises(pkg.InvalidArgument, match="step_idx"):
        pkg.skip_residual_add_steps(ctx, [(d, src.cuda())], 2, table, 2)
    with pytest.raises(pkg.InvalidArgument, match="scales"):
        pkg.skip_residual_add_steps(ctx, [(d, src.cuda())], 2, table[:, :4].contiguous(), 0)
    assert torch.equal(d.cpu(), buf)
