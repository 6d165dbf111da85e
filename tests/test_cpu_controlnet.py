"""ControlNet skip residuals without a GPU: the host-only entries against the reference of tests/controlnet_ref.py, the reference against the oracle
it restates, and the fixture of the GPU tests held to "the control net and its hint matter"."""
import ctypes

import pytest
import torch

from oracle import config as OC, model as OM
from util import rel_err, to_pkg_cfg, unet_weights
from test_gpu_models import FWD_TOL
import controlnet_ref as CR

FWD_TOL_F16 = FWD_TOL[1]


class Fixture:
    """UNet seed 0, control net seed 1, B = 2, the inputs of test_gpu_lora.Tiny, t = [999, 1], block hints of seeds 1 and 2"""

    def __init__(self):
        self.ocfg = OC.tiny_config()
        self.W, self.Wc = unet_weights(self.ocfg), CR.control_weights(self.ocfg, 1)
        B = 2
        self.x = torch.from_numpy(OC.arb_tensor(B, 4, 16, 16))
        self.context = torch.from_numpy(OC.arb_tensor(B, 5, self.ocfg.context_dim))
        self.y = torch.from_numpy(OC.arb_tensor(B, self.ocfg.adm_in_channels))
        self.t = torch.tensor([999, 1])
        self.base = OM.unet_forward(self.ocfg, self.W, self.x, self.t, self.context, self.y)
        self.res = {s: CR.control_forward(self.ocfg, self.Wc, self.x, self.t, self.context, self.y, CR.block_hint(B, 128, 128, s)) for s in (1, 2)}

    def controlled(self, residuals, scale):
        return CR.controlled_unet_forward(self.ocfg, self.W, self.x, self.t, self.context, self.y, residuals, scale)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def test_skip_shapes_equal_the_reference(pkg):
    ocfg = OC.tiny_config()
    cfg = to_pkg_cfg(pkg, ocfg)
    c = cfg.to_c()
    inp, _, _ = OC.unet_block_plan(ocfg)
    assert pkg.lib().sdxl_unet_skip_count(ctypes.byref(c)) == len(inp) + 1
    for H, W in ((16, 16), (8, 24)):
        assert pkg.unet_skip_shapes(cfg, H, W) == CR.skip_shapes(ocfg, H, W)
    base = OC.sdxl_base_config()
    shapes = pkg.unet_skip_shapes(to_pkg_cfg(pkg, base), 128, 128)
    assert shapes == CR.skip_shapes(base, 128, 128) and len(shapes) == 10 and shapes[0] == (320, 128, 128) and shapes[-1] == (1280, 32, 32)


def test_reference_restates_the_oracle(fx):
    # no residuals: the operations of OM.unet_forward, bit for bit; residuals at scale 0: the base output as values
    assert torch.equal(fx.controlled(None, 1.0), fx.base)
    assert torch.equal(fx.controlled(fx.res[1], 0.0), fx.base)
    assert [tuple(r.shape[1:]) for r in fx.res[1]] == CR.skip_shapes(fx.ocfg, 16, 16)
    n_unet, n_ctrl = len(OC.unet_param_specs(fx.ocfg)), len(CR.controlnet_param_specs(fx.ocfg))
    assert (n_unet, n_ctrl) == (717, 369)


def test_fixture_matters(fx):
    # a tolerance that an un-controlled or a hint-blind engine would meet as well shows nothing
    c1, c2 = fx.controlled(fx.res[1], 1.0), fx.controlled(fx.res[2], 1.0)
    moved, hints = rel_err(c1, fx.base), rel_err(c2, c1)
    per_tensor = [rel_err(a, b) for a, b in zip(fx.res[2], fx.res[1])]
    print(f"scale 1 moves the output by {moved:.3f}; the two hints' outputs differ by {hints:.3f}; residual tensors differ by {min(per_tensor):.3f} .. {max(per_tensor):.3f}")
    assert moved >= 100 * FWD_TOL_F16
    assert hints >= 100 * FWD_TOL_F16
    assert min(per_tensor) > 0.4
    half = fx.controlled(fx.res[1], 0.5)
    assert rel_err(half, c1) >= 10 * FWD_TOL_F16 and rel_err(half, fx.base) >= 10 * FWD_TOL_F16      # the scale matters as well


def test_host_only_argument_checks(pkg):
    cfg = to_pkg_cfg(pkg, OC.tiny_config())
    c = cfg.to_c()
    chw = (ctypes.c_int64 * 3)()
    n = pkg.lib().sdxl_unet_skip_count(ctypes.byref(c))
    l = pkg.lib()
    assert l.sdxl_unet_skip_shape(ctypes.byref(c), 0, 16, 16, chw) == 0
    for index, H, W, word in ((-1, 16, 16, "index"), (n, 16, 16, "index"), (0, 0, 16, "multiples"), (0, 16, 10, "multiples"), (0, -8, 16, "multiples")):
        assert l.sdxl_unet_skip_shape(ctypes.byref(c), index, H, W, chw) == 1, (index, H, W)
        assert word in l.sdxl_last_error().decode()
    assert l.sdxl_unet_skip_shape(ctypes.byref(c), 0, 16, 16, None) == 1
    with pytest.raises(pkg.InvalidArgument):
        pkg.unet_skip_shapes(cfg, 16, 10)


def test_param_specs_equal_the_reference(pkg):
    import numpy as np
    for ocfg, count in ((OC.tiny_config(), 369), (OC.sdxl_base_config(), None)):
        got = pkg.controlnet_param_specs(pkg.ControlNetConfig(to_pkg_cfg(pkg, ocfg)))
        ref = CR.controlnet_param_specs(ocfg)
        assert len(got) == len(ref) and (count is None or len(got) == count)
        for g, r in zip(got, ref):
            assert (g.name, tuple(g.shape), g.kind) == (r.name, tuple(r.shape), r.kind)
            assert np.float32(g.scale) == r.scale and np.float32(g.mean) == r.mean, g.name
    names = [g.name for g in got]
    assert not any(n.startswith(("output_blocks", "norm_out", "conv_out")) for n in names)
    assert names[-2:] == ["middle_block_out.weight", "middle_block_out.bias"]
    hint = [g for g in got if g.name.startswith("input_hint_block.") and g.name.endswith(".weight")]
    assert [tuple(g.shape) for g in hint] == [(16, 3, 3, 3), (16, 16, 3, 3), (32, 16, 3, 3), (32, 32, 3, 3), (96, 32, 3, 3), (96, 96, 3, 3), (256, 96, 3, 3), (320, 256, 3, 3)]


def test_controlnet_config_checks(pkg):
    l = pkg.lib()
    c = pkg.ControlNetConfig(to_pkg_cfg(pkg, OC.tiny_config())).to_c()
    d = type(c)()
    l.sdxl_controlnet_config_default(ctypes.byref(c.unet), ctypes.byref(d))
    assert bytes(d) == bytes(c)
    assert l.sdxl_controlnet_param_count(ctypes.byref(c)) == 369
    assert l.sdxl_controlnet_param_spec(ctypes.byref(c), 369, None, None, None, None, None, None) == 1      # SDXL_ERR_INVALID
    assert l.sdxl_controlnet_param_spec(ctypes.byref(c), -1, None, None, None, None, None, None) == 1
    c.hint_channels[2] = 12
    assert l.sdxl_controlnet_param_count(ctypes.byref(c)) == -1 and "hint_channels" in l.sdxl_last_error().decode()
    assert l.sdxl_controlnet_param_count(None) == -1
