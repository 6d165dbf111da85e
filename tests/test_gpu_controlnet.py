"""ControlNet on the GPU: the one-launch add op against fp64, the control net alone, the UNet with residuals given by the caller, both in series
(ControlNet.forward into UNet.forward_residuals) and the refusals, against the reference of tests/controlnet_ref.py.  Tiny configuration at
16 x 16; the CPU references are computed once per module."""
import numpy as np
import pytest
import torch

from oracle import config as OC, model as OM
from util import rel_err, rounding_slack, seeded, to_pkg_cfg, unet_weights
from test_gpu_models import FWD_TOL
import controlnet_ref as CR
from skip_add_ref import skip_add_expected

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- 1. the add op
# (rows, C, ld, col_off): one 16-byte chunk; an odd row count in the last third of a wider buffer; an SDXL width; an odd row count in the upper half
SEGS = [(1, 8, 8, 0), (37, 64, 192, 128), (256, 320, 960, 640), (4099, 64, 128, 64)]
TABLES = {
    1: [SEGS[3]],
    3: SEGS[:3],      # 1, 37 and 256 rows: the second and third segments start inside a workgroup
    16: [SEGS[i % 4] if i < 4 else (SEGS[i % 4][0] + 3 * i, ) + SEGS[i % 4][1:] for i in range(16)],
    # the grid is capped at 2048 workgroups of 256 lanes, one 16-byte chunk each: 16411 x 320 is 1.25 (f16) / 2.5 (fp32) trips of the grid-stride
    # loop, and the lanes of the last trip cross into the small segment behind it
    "trips": [(16411, 320, 320, 0), (3, 8, 24, 8)],
}


def _spacing32(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23.0)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _table(n, tdt):
    bufs, srcs = [], []
    for i, (rows, C, ld, off) in enumerate(TABLES[n]):
        bufs.append(seeded(rows, ld, seed=100 + i).to(tdt))
        srcs.append(seeded(rows, C, seed=200 + i).to(tdt))
    return bufs, srcs


@pytest.mark.parametrize("scale", [1.0, -0.37, 0.0])
@pytest.mark.parametrize("n_seg", [1, 3, 16, "trips"])
@pytest.mark.parametrize("tdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_add_op_against_fp64(pkg, ctx, tdt, n_seg, scale):
    bufs, srcs = _table(n_seg, tdt)

    def run():
        d = [b.cuda() for b in bufs]
        s = [x.cuda() for x in srcs]
        pkg.skip_residual_add(ctx, [(b[:, off:off + C], x) for b, x, (_, C, _, off) in zip(d, s, TABLES[n_seg])], scale)
        return [b.cpu() for b in d]

    outs, again = run(), run()
    s64 = float(np.float32(scale))
    worst = 0.0
    for out, rep, buf, src, (rows, C, ld, off) in zip(outs, again, bufs, srcs, TABLES[n_seg]):
        assert torch.equal(out.view(torch.int16 if tdt == torch.float16 else torch.int32), rep.view(torch.int16 if tdt == torch.float16 else torch.int32)), "two runs differ"
        keep = torch.ones(ld, dtype=torch.bool)
        keep[off:off + C] = False
        assert torch.equal(out[:, keep], buf[:, keep]), "columns outside the slice changed"
        ref = buf[:, off:off + C].double() + s64 * src.double()      # (the product is exact in fp64; the kernel rounds the exact sum once to fp32)
        got = out[:, off:off + C].double()
        if tdt == torch.float32:
            bound = 0.5 * _spacing32(ref) * (1 + 2.0 ** -20)
            err = (got - ref).abs()
        else:      # one more rounding, fp32 -> f16: f16(ref), or its neighbour where the fp32 value may sit across a rounding midpoint
            h, slack = rounding_slack(ref, 0.5 * _spacing32(ref))
            bound, err = slack, (got - h).abs()
        assert bool((err <= bound).all()), f"segment {(rows, C, ld, off)}: max err {err.max():.3e}"
        worst = max(worst, (got - ref).abs().max().item())
        # the bits: one correctly rounded fp32 fma and one rounding to the type, computed on the CPU (the one-scalar form does not skip at scale 0)
        old = buf[:, off:off + C].numpy()
        want = torch.from_numpy(skip_add_expected(old, [src.numpy()], [scale], old.dtype, skip_zero=False))
        differ = int((_bits(out[:, off:off + C]) != _bits(want)).sum())
        print(f"segment {(rows, C, ld, off)}: {differ} of {want.numel()} elements differ from the expected bits")
        assert differ == 0
        if scale == 0.0:
            assert torch.equal(out, buf), "scale 0 changed the destination"
        else:
            assert not torch.equal(out[:, off:off + C], buf[:, off:off + C])
    print(f"skip_residual_add {n_seg} segments {tdt} scale {scale}: max |out - fp64| {worst:.3e}")


def test_add_op_scale_zero_is_still_the_fma(pkg, ctx):
    """dst = round(fma(scale, src, dst)) at every scale: the one-scalar entry has no rule for scale 0 (the table forms do), so a NaN source
    reaches its rows of the destination and all other rows keep their bits"""
    rows, C, ld, off = SEGS[1]
    buf, src = seeded(rows, ld, seed=5).half(), seeded(rows, C, seed=6).half()
    src[11] = float("nan")
    d = buf.cuda()
    pkg.skip_residual_add(ctx, [(d[:, off:off + C], src.cuda())], 0.0)
    out = d.cpu()
    assert bool(torch.isnan(out[11, off:off + C]).all()), "0 * NaN + dst must be NaN"
    want = buf.clone()
    want[:, off:off + C] = torch.from_numpy(skip_add_expected(buf[:, off:off + C].numpy(), [src.numpy()], [0.0], np.float16, skip_zero=False))
    live = torch.arange(rows) != 11
    assert torch.equal(_bits(out[live]), _bits(want[live])) and torch.equal(_bits(out[live]), _bits(buf[live]))
    assert torch.equal(_bits(out[11, :off]), _bits(buf[11, :off])) and torch.equal(_bits(out[11, off + C:]), _bits(buf[11, off + C:]))


@pytest.mark.parametrize("tdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_add_op_refuses_misaligned_segments(pkg, ctx, tdt):
    buf, src = seeded(37, 192, seed=1).to(tdt), seeded(37, 64, seed=2).to(tdt)
    good = seeded(5, 64, seed=3).to(tdt)
    scale_dev = torch.tensor([1.0], device="cuda")
    for what, view, s in (("slice starts off a 16-byte boundary", lambda d: d[:, 1:65], src),
                          ("C % 8 != 0", lambda d: d[:, 0:12], src[:, :12].contiguous()),
                          ("row pitch off a 16-byte boundary", lambda d: d.reshape(-1)[:37 * 190].view(37, 190)[:, 0:64], src)):
        d, g = buf.cuda(), good.cuda()
        with pytest.raises(pkg.InvalidArgument) as e:      # the bad segment is second: the good one in front of it must stay untouched as well
            pkg.skip_residual_add(ctx, [(g, good.cuda()), (view(d), s.cuda())], scale_dev)
        print(f"{what}: {e.value}")
        assert torch.equal(d.cpu(), buf) and torch.equal(g.cpu(), good), what
    with pytest.raises(pkg.InvalidArgument):
        pkg.skip_residual_add(ctx, [(good.cuda(), good.cuda())] * 17, 1.0)


# ---------------------------------------------------------------------------------------------------------------- 3. the UNet with given residuals
class Tiny:
    """UNet seed 0, control net seed 1, B = 2, the inputs of test_gpu_lora.Tiny, t = [999, 1], block hints of seed 1"""

    def __init__(self, pkg):
        self.ocfg = OC.tiny_config()
        self.cfg = to_pkg_cfg(pkg, self.ocfg)
        self.W, self.Wc = unet_weights(self.ocfg), CR.control_weights(self.ocfg, 1)
        B = 2
        self.x = torch.from_numpy(OC.arb_tensor(B, 4, 16, 16))
        self.context = torch.from_numpy(OC.arb_tensor(B, 5, self.ocfg.context_dim))
        self.y = torch.from_numpy(OC.arb_tensor(B, self.ocfg.adm_in_channels))
        self.t = torch.tensor([999, 1], dtype=torch.int32)
        self.hint = CR.block_hint(B, 128, 128, 1)
        self.base = OM.unet_forward(self.ocfg, self.W, self.x, self.t.long(), self.context, self.y)
        self.res = CR.control_forward(self.ocfg, self.Wc, self.x, self.t.long(), self.context, self.y, self.hint)
        self.g = CR.embed_hint(self.Wc, self.hint)
        self.ccfg = pkg.ControlNetConfig(self.cfg)
        self.controlled = {s: CR.controlled_unet_forward(self.ocfg, self.W, self.x, self.t.long(), self.context, self.y, self.res, s) for s in (1.0, 0.5)}

    def args(self, n=2):
        return self.x[:n].cuda(), self.t[:n].cuda(), self.context[:n].cuda(), self.y[:n].cuda()

    def res_dev(self, n=2):
        return [r[:n].cuda() for r in self.res]


@pytest.fixture(scope="module")
def tiny(pkg):
    return Tiny(pkg)


@pytest.mark.parametrize("dtype", [0, 1, 3])
def test_unet_with_given_residuals(pkg, ctx, tiny, dtype):
    u = pkg.UNet(ctx, tiny.cfg, dtype, seed=0)
    outs = [u.forward_residuals(*tiny.args(), tiny.res_dev(), 1.0).cpu() for _ in range(3)]      # eager, capture, replay
    half = u.forward_residuals(*tiny.args(), tiny.res_dev(), 0.5).cpu()      # another scale: the same graph
    again = u.forward_residuals(*tiny.args(), tiny.res_dev(), 1.0).cpu()
    e1, e05, moved = rel_err(outs[0], tiny.controlled[1.0]), rel_err(half, tiny.controlled[0.5]), rel_err(outs[0], tiny.base)
    print(f"dtype {dtype}: given residuals scale 1 rel err {e1:.3e}, scale 0.5 {e05:.3e} (bar {FWD_TOL[dtype]:.1e}); scale 1 moves the output by {moved:.3f}")
    assert moved >= 100 * FWD_TOL[1], "the residuals do not matter: the tolerance would show nothing"
    assert e1 < FWD_TOL[dtype] and e05 < FWD_TOL[dtype]
    for o in outs[1:] + [again]:
        assert torch.equal(o, outs[0]), "eager / capture / replay differ"
    # scale 0, explicit detach and the plain entry: the plain forward of a handle that never had residuals
    plain = pkg.UNet(ctx, tiny.cfg, dtype, seed=0).forward(*tiny.args()).cpu()
    assert torch.equal(u.forward_residuals(*tiny.args(), tiny.res_dev(), 0.0).cpu(), plain), "scale 0"
    assert torch.equal(u.forward_residuals(*tiny.args(), None).cpu(), plain), "residuals=None"
    assert torch.equal(u.forward_residuals(*tiny.args(), tiny.res_dev(), 1.0).cpu(), outs[0]), "attached again"
    for _ in range(2):
        assert torch.equal(u.forward(*tiny.args()).cpu(), plain), "forward() after residuals"
    # batch independence: entry 0 of the batch-2 call is the batch-1 call
    one = u.forward_residuals(*tiny.args(1), tiny.res_dev(1), 1.0).cpu()
    assert torch.equal(one, outs[0][:1])


# ---------------------------------------------------------------------------------------------------------------- 6. errors
def test_residual_refusals_leave_the_handle_as_it_was(pkg, ctx, tiny):
    fresh = pkg.UNet(ctx, tiny.cfg, 0, seed=0).forward(*tiny.args()).cpu()
    u = pkg.UNet(ctx, tiny.cfg, 0, seed=0)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(pkg.InvalidArgument, match="finite"):
            u.forward_residuals(*tiny.args(), tiny.res_dev(), bad)
    with pytest.raises(pkg.InvalidArgument, match="shapes"):
        u.forward_residuals(*tiny.args(), tiny.res_dev()[:-1], 1.0)
    assert torch.equal(u.forward(*tiny.args()).cpu(), fresh)
    # split CFG and skip residuals: refused at whichever call would create the combination, naming both
    u.set_split_cfg(True)
    with pytest.raises(pkg.InvalidArgument, match="(?s)split.*residual|residual.*split"):
        u.forward_residuals(*tiny.args(), tiny.res_dev(), 1.0)
    assert torch.equal(u.forward(*tiny.args()).cpu(), fresh)      # (split CFG is bit-identical to the batched chain)
    u.set_split_cfg(False)
    ctrl = u.forward_residuals(*tiny.args(), tiny.res_dev(), 1.0).cpu()
    with pytest.raises(pkg.InvalidArgument, match="(?s)split.*residual|residual.*split"):
        u.set_split_cfg(True)
    assert torch.equal(u.forward_residuals(*tiny.args(), tiny.res_dev(), 1.0).cpu(), ctrl)
    assert torch.equal(u.forward(*tiny.args()).cpu(), fresh)
    # a dtype mode no test covers is refused by name
    u2 = pkg.UNet(ctx, tiny.cfg, pkg.DTYPE_F16_F32RES, seed=0)
    with pytest.raises(pkg.InvalidArgument, match="SDXL_DTYPE_F16_F32RES"):
        u2.forward_residuals(*tiny.args(), tiny.res_dev(), 1.0)
    u3 = pkg.UNet(ctx, tiny.cfg, pkg.DTYPE_F32_SPLIT_F16W, seed=0)      # (on these weights the mode falls back to F32_SPLIT's arithmetic: still refused)
    with pytest.raises(pkg.InvalidArgument, match="SDXL_DTYPE_F32_SPLIT_F16W"):
        u3.forward_residuals(*tiny.args(), tiny.res_dev(), 1.0)


# ---------------------------------------------------------------------------------------------------------------- 2. the control net alone
@pytest.mark.parametrize("dtype", [0, 1, 3])
def test_control_net_alone(pkg, ctx, tiny, dtype):
    # an encoder-only forward: the class FWD_TOL was measured on
    c = pkg.ControlNet(ctx, tiny.ccfg, dtype, seed=1)
    eg = rel_err(c.embed_hint(tiny.hint.cuda()).cpu(), tiny.g)
    runs = [[r.cpu() for r in c.forward(*tiny.args(), tiny.hint.cuda())] for _ in range(3)]      # eager, capture, replay
    errs = [rel_err(o, r) for o, r in zip(runs[0], tiny.res)]
    print(f"dtype {dtype}: embed_hint rel err {eg:.3e}, residual tensors {min(errs):.3e} .. {max(errs):.3e} (bar {FWD_TOL[dtype]:.1e})")
    assert len(runs[0]) == len(tiny.res) == 10
    assert eg < FWD_TOL[dtype] and max(errs) < FWD_TOL[dtype]
    for run in runs[1:]:
        for o, a in zip(runs[0], run):
            assert torch.equal(o, a), "eager / capture / replay differ"


def test_control_net_non_square(pkg, ctx, tiny):
    B, H, W = 2, 8, 24
    x = torch.from_numpy(OC.arb_tensor(B, 4, H, W))
    hint = CR.block_hint(B, 8 * H, 8 * W, 3)
    ref = CR.control_forward(tiny.ocfg, tiny.Wc, x, tiny.t.long(), tiny.context, tiny.y, hint)
    c = pkg.ControlNet(ctx, tiny.ccfg, 0, seed=1)
    out = c.forward(x.cuda(), tiny.t.cuda(), tiny.context.cuda(), tiny.y.cuda(), hint.cuda())
    assert [tuple(o.shape[1:]) for o in out] == pkg.unet_skip_shapes(tiny.cfg, H, W)
    errs = [rel_err(o.cpu(), r) for o, r in zip(out, ref)]
    print(f"8 x 24 latent, 64 x 192 hint: residual tensors {min(errs):.3e} .. {max(errs):.3e}")
    assert max(errs) < FWD_TOL[0]
    assert rel_err(c.embed_hint(hint.cuda()).cpu(), CR.embed_hint(tiny.Wc, hint)) < FWD_TOL[0]


# ---------------------------------------------------------------------------------------------------------------- 4. both in series
# two networks in a chain: not the class FWD_TOL was measured on.  Bound = 2 x the rel_err measured on the MI355X (profiles/controlnet_tests.txt),
# the margin the project's other measured tolerances carry; it must not exceed 2 x FWD_TOL.
SERIES_MEASURED = {0: 2.181e-6, 1: 1.614e-3, 3: 1.818e-6}      # -> bounds 4.4e-6 / 3.2e-3 / 3.6e-6, under 2 x FWD_TOL = 2e-5 / 9e-3 / 2e-5


@pytest.mark.parametrize("dtype", [0, 1, 3])
def test_control_net_and_unet_in_series(pkg, ctx, tiny, dtype):
    c = pkg.ControlNet(ctx, tiny.ccfg, dtype, seed=1)
    u = pkg.UNet(ctx, tiny.cfg, dtype, seed=0)
    outs = []
    for _ in range(3):
        r = c.forward(*tiny.args(), tiny.hint.cuda())
        outs.append(u.forward_residuals(*tiny.args(), r, 1.0).cpu())
    e = rel_err(outs[0], tiny.controlled[1.0])
    bound = 2 * SERIES_MEASURED[dtype]
    print(f"dtype {dtype}: control net + UNet in series rel err {e:.3e} (bound {bound:.3e}, 2 x FWD_TOL {2 * FWD_TOL[dtype]:.1e})")
    assert bound <= 2 * FWD_TOL[dtype]
    assert e < bound
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])


# ---------------------------------------------------------------------------------------------------------------- 6. errors of the control net
def test_control_net_refusals(pkg, ctx, tiny):
    with pytest.raises(pkg.InvalidArgument, match="SDXL_DTYPE"):
        pkg.ControlNet(ctx, tiny.ccfg, pkg.DTYPE_F16_F32RES, seed=1)
    with pytest.raises(pkg.InvalidArgument, match="SDXL_DTYPE"):
        pkg.ControlNet(ctx, tiny.ccfg, pkg.DTYPE_F32_SPLIT_MIX, seed=1)
    rcfg = to_pkg_cfg(pkg, OC.tiny_refiner_config())
    with pytest.raises(pkg.InvalidArgument, match="refiner"):
        pkg.ControlNet(ctx, pkg.ControlNetConfig(rcfg), 0, seed=1)
    c = pkg.ControlNet(ctx, tiny.ccfg, 0, seed=1)
    good = [r.cpu() for r in c.forward(*tiny.args(), tiny.hint.cuda())]
    with pytest.raises(pkg.InvalidArgument, match="hint"):      # a hint that is not 8 x the latent
        c.forward(*tiny.args(), tiny.hint[:, :, :120].cuda())
    with pytest.raises(pkg.InvalidArgument, match="8 x"):
        c.embed_hint(tiny.hint[:, :, :60].cuda())
    again = [r.cpu() for r in c.forward(*tiny.args(), tiny.hint.cuda())]
    assert all(torch.equal(a, b) for a, b in zip(good, again))
