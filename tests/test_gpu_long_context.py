"""The UNet on a long context (n_ctx = 154 / 231: two / three 77-token chunks): the f16 engine keeps the cross-attention inside the query
projection's launch (csrc/igemm_wreg.hip, long XA form) where the knob "xattn_long" allows it, and falls back to projection + attention kernel
where it does not; the split-operand modes keep that fallback above 96 keys.  tiny_config at a 32 x 32 latent: both transformer levels have whole
64-row blocks per entry (16^2 = 256 and 8^2 = 64 rows) and widths 128 / 256, so every cross-attention of the net can take the fused form."""
import pytest
import torch

from oracle import config as OC, model as OM, pipeline as OP
from test_gpu_models import FWD_TOL, LAT_REL_F16, _cond, _pkg_cond, weights_for
from util import max_abs, rel_err, to_pkg_cfg

pytestmark = pytest.mark.gpu

_REF = {}


def _problem(n_ctx, dtype=1, pkg=None):
    """inputs and the oracle's forward for one context length (and weight set), computed once"""
    ocfg = OC.tiny_config()
    f16w = dtype in (5, 6, 7)
    if (n_ctx, f16w) not in _REF:
        W, _ = weights_for(pkg, ocfg, dtype)
        x = torch.from_numpy(OC.arb_tensor(2, 4, 32, 32))
        context = torch.from_numpy(OC.arb_tensor(2, n_ctx, ocfg.context_dim))
        y = torch.from_numpy(OC.arb_tensor(2, ocfg.adm_in_channels))
        t = torch.tensor([999, 1], dtype=torch.int32)
        _REF[(n_ctx, f16w)] = (x, t, context, y, OM.unet_forward(ocfg, W, x, t.long(), context, y))
    return _REF[(n_ctx, f16w)]


class _Long:
    """the process-wide knob "xattn_long" for the duration of a block, restored to its default"""

    def __init__(self, pkg, value):
        self.pkg, self.value = pkg, value

    def __enter__(self):
        self.pkg.debug_set("xattn_long", self.value)

    def __exit__(self, *exc):
        self.pkg.debug_set("xattn_long", 1)
        return False


@pytest.mark.parametrize("n_ctx", [154, 231])
def test_long_context_forward_fused_and_unfused(pkg, ctx, n_ctx):
    ocfg = OC.tiny_config()
    x, t, context, y, ref = _problem(n_ctx, 1, pkg)
    dev = [a.cuda() for a in (x, t, context, y)]
    outs, attn = {}, {}
    for knob in (1, 0):
        u = pkg.UNet(ctx, to_pkg_cfg(pkg, ocfg), 1, seed=0)
        with _Long(pkg, knob):
            o = [u.forward(*dev).cpu() for _ in range(3)]      # eager, capture, replay
            attn[knob] = u.profile(2, 32, 32)["attention"][1]
        assert torch.equal(o[0], o[1]) and torch.equal(o[1], o[2]), "hipGraph replay differs from the eager run"
        outs[knob] = o[0]
    e1, e0 = rel_err(outs[1], ref), rel_err(outs[0], ref)
    print(f"long context n_ctx={n_ctx}: fused vs oracle {e1:.3e}, un-fused vs oracle {e0:.3e}, between them {rel_err(outs[1], outs[0]):.3e}; "
          f"attention-class launches {attn[1]} fused / {attn[0]} un-fused")
    assert e1 < FWD_TOL[1] and e0 < FWD_TOL[1]
    # one self-attention per transformer block when fused; the cross-attention's own launch on top when not: the long form is what ran
    assert attn[1] > 0 and attn[0] == 2 * attn[1]


def test_long_context_knob_is_read_when_the_context_is_set(pkg, ctx):
    """one handle, the knob flipped between forwards: the context image is packed or dropped with it, and each setting reproduces its bits"""
    ocfg = OC.tiny_config()
    x, t, context, y, _ = _problem(154, 1, pkg)
    dev = [a.cuda() for a in (x, t, context, y)]
    u = pkg.UNet(ctx, to_pkg_cfg(pkg, ocfg), 1, seed=0)
    on = u.forward(*dev).cpu()
    with _Long(pkg, 0):
        off = [u.forward(*dev).cpu() for _ in range(3)]
    again = [u.forward(*dev).cpu() for _ in range(3)]
    fresh = pkg.UNet(ctx, to_pkg_cfg(pkg, ocfg), 1, seed=0)
    with _Long(pkg, 0):
        off_fresh = fresh.forward(*dev).cpu()
    assert all(torch.equal(o, off_fresh) for o in off)
    assert all(torch.equal(o, on) for o in again)


def test_long_context_sample_latent(pkg, ctx):
    ocfg = OC.tiny_config()
    res = (256, 256)
    c, oc = _cond(ocfg, 1, res, n_ctx=154)
    noise = torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(40))
    W, wseed = weights_for(pkg, ocfg, 1)
    ref = OP.Diffuser(ocfg, W, OC.alphas_cumprod()).sample_latent(oc, 7.5, 4, noise)
    d = pkg.Diffuser(ctx, to_pkg_cfg(pkg, ocfg), 1, seed=wseed)
    out = d.sample_latent(_pkg_cond(pkg, c, res), 7.5, 4, noise.cuda()).cpu()
    e = max_abs(out, ref)
    print(f"long context sample_latent n_ctx=154: latent max-abs err {e:.3e} (|latent| max {ref.abs().max():.2f})")
    assert torch.isfinite(out).all() and e < LAT_REL_F16 * float(ref.abs().max())


@pytest.mark.parametrize("dtype", [3, 5])
def test_split_operand_modes_keep_the_unfused_fallback(pkg, ctx, dtype):
    ocfg = OC.tiny_config()
    x, t, context, y, ref = _problem(154, dtype, pkg)
    u = pkg.UNet(ctx, to_pkg_cfg(pkg, ocfg), dtype, seed=weights_for(pkg, ocfg, dtype)[1])
    out = u.forward(x.cuda(), t.cuda(), context.cuda(), y.cuda()).cpu()
    e = rel_err(out, ref)
    print(f"long context n_ctx=154 dtype={dtype}: rel err {e:.3e}")
    assert e < FWD_TOL[dtype]
