"""The per-step sampler kernel, bit for bit: every case of tests/golden/sampler_step_bits.npz again through sdxl_sampler_step_replay (the
trajectory without the UNet: table, initial launch, per iteration the rescale factors and the update, with the noise predictions given).

The fixture was recorded from the three kernels the project had at commit 456ca47 (tools/record_sampler_step_fixture.py; layout, cases and the note
on toolchains in tests/sampler_step_cases.py).  A case that fails here means a rounding of the kernel changed: read the kernel, never re-record."""
import os

import numpy as np
import pytest
import torch

import sampler_step_cases as C

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_step_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", C.all_cases(), ids=C.case_name)
def test_replay_equals_the_record(pkg, ctx, golden, case):
    name = C.case_name(case)
    inp = {k: golden[f"in/{C.shape_key(case['shape'])}/{k}"] for k in ("eps", "latent0", "reference", "mask", "step_noise", "seeds")}
    packed, h_lat, h_ts = C.run_case(pkg, ctx, case, inp, golden["in/alphas"])
    want = torch.from_numpy(golden["out/" + name])
    for what, got, ref in zip(("final latent", "UNet-input copy", "history"), C.unpack(case, packed), C.unpack(case, want)):
        if ref is not None:
            assert torch.equal(got, ref), f"{name}: {what} differs in {int((got != ref).sum())} of {ref.numel()} values, max-abs {float((got - ref).abs().max()):.3e}"
    assert torch.equal(packed.view(torch.int32), want.view(torch.int32)), f"{name}: equal values, different bits (a zero's sign)"
    assert [h_lat, h_ts] == [str(v) for v in golden["sha/" + name]], f"{name}: the per-iteration latents or the timesteps differ"


def test_argument_errors(pkg, ctx):
    """SDXL_ERR_INVALID with a message that names the complaint; the same arguments without the fault run"""
    a = pkg.default_alphas_cumprod()
    n, h, w, iters = 2, 8, 17, 4
    z = lambda *s: torch.zeros(*s, device="cuda")
    ok = dict(alphas=a, n_steps=4, step_start=0, eps=z(iters, 2 * n, h * w, 4), latent0=z(n, 4, h, w))
    mask = torch.ones(n, 4, h, w, dtype=torch.uint8, device="cuda")
    refused = [
        (dict(eps=z(iters, 18, h * w, 4), latent0=z(9, 4, h, w)), r"1\.\.8"),
        (dict(mask=mask), "reference"),
        (dict(mask=mask, reference=z(n, 4, h, w)), "step_noise"),
        (dict(eta=0.5), "seeds"),
        (dict(guidance=pkg.make_guidance(scales=[1.0, 2.0, 3.0])), "n_scales"),
        (dict(guidance=pkg.make_guidance(rescale=0.5), single=True, eps=z(iters, n, h * w, 4)), "guidance"),
        (dict(guidance=pkg.make_guidance(t_range=(100, 900)), single=True, eps=z(iters, n, h * w, 4)), "guidance"),
        (dict(guidance=pkg.make_guidance(rescale=1.5)), "rescale"),
        (dict(solver=7), "solver"),
    ]
    for options, word in refused:
        with pytest.raises(pkg.InvalidArgument, match=word):
            pkg.sampler_step_replay(ctx, **{**ok, **options})
    latents, _, unet_in, ts = pkg.sampler_step_replay(ctx, **ok)       # and the accepted call runs
    assert latents.shape == (iters + 1, n, 4, h, w) and ts.cpu().tolist() == [999.0, 749.0, 499.0, 249.0, 0.0]
    assert pkg.lib().sdxl_sampler_step_replay(ctx.h, None, None) == 1
