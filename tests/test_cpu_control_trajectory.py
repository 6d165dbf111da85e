"""Control nets in a trajectory, the parts that need no GPU: the scale table (sdxl_control_scale_table) against the restatement of
tests/control_traj_ref.py, and the fixture a trajectory test of the Diffuser wiring stands on -- the fp32 CPU reference trajectory with control
seed 1 -- held to "it matters and it behaves"."""
import numpy as np
import pytest
import torch

import control_traj_ref as TR
import controlnet_ref as CR
import solver_ref as R
from oracle import config as OC
from test_gpu_models import LAT_REL_F16, _cond
from util import seeded, unet_weights

ALPHAS = OC.alphas_cumprod()
TS8 = [t for t, _, _ in R.schedule(ALPHAS, 8)]      # 999, 874, ..., 124
# the conditioning scale for trajectory tests, chosen by test_fixture_matters_and_behaves
CONTROL_SCALE = 1.0

TABLE_CASES = {
    "default": dict(),
    "scale": dict(scale=0.625),
    "per_entry": dict(scales=[1.0, -0.37]),
    "not_first": dict(t_range=(0, 900)),
    "not_last": dict(t_range=(200, 999)),
    "middle_only": dict(t_range=(300, 700)),
    "not_middle_nor_last": dict(scale=0.5, t_range=(874, 999)),
    "no_iteration": dict(t_range=(1000, 2000)),
    "cond_only": dict(cond_only=True, scales=[0.5, 2.0]),
    "cond_only_interval": dict(cond_only=True, t_range=(300, 700)),
}


@pytest.mark.parametrize("case", list(TABLE_CASES))
@pytest.mark.parametrize("single", [False, True], ids=["pair", "single"])
def test_scale_table_equals_the_restatement(pkg, case, single):
    k = TABLE_CASES[case]
    if single and k.get("cond_only"):
        with pytest.raises(pkg.InvalidArgument, match="cond_only"):
            pkg.control_scale_table(pkg.make_control(**k), 2, TS8, single_branch=True)
        return
    got = pkg.control_scale_table(pkg.make_control(**k), 2, TS8, single_branch=single)
    want = TR.scale_table(2, TS8, single=single, **k)
    assert got.dtype == np.float32 and got.shape == (9, 8)
    assert np.array_equal(got, want), f"{case}:\n{got}\n{want}"
    assert not got[8].any(), "the sentinel row is not zero"
    assert not got[:, (2 if single else 4):].any(), "entries behind the batch are not zero"
    if case in ("not_first", "middle_only"):
        assert not got[0].any() and got[3].any()
    if case in ("not_last", "middle_only", "not_middle_nor_last"):
        assert not got[7].any()
    if case == "not_middle_nor_last":
        assert got[0].any() and got[1].any() and not got[2:].any()
    if case == "no_iteration":
        assert not got.any()


def test_scale_tables_of_two_nets_differ_as_their_options_do(pkg):
    """K = 2: a table [iters + 1][K][8] for sdxl_skip_residual_add_steps_multi is these two, row by row"""
    a, b = dict(scales=[1.0, 0.25], t_range=(499, 999)), dict(scale=-0.5, cond_only=True, t_range=(0, 600))
    ta, tb = (pkg.control_scale_table(pkg.make_control(**k), 2, TS8) for k in (a, b))
    assert np.array_equal(ta, TR.scale_table(2, TS8, **a)) and np.array_equal(tb, TR.scale_table(2, TS8, **b))
    both = np.stack([ta, tb], axis=1)
    assert both.shape == (9, 2, 8)
    assert both[0, 0, :4].tolist() == [1.0, 0.25, 1.0, 0.25] and not both[0, 1].any()      # 999: net 0 alone
    assert not both[7, 0].any() and both[7, 1, :4].tolist() == [-0.5, -0.5, 0.0, 0.0]      # 124: net 1 alone, conditional entries
    assert both[3, 0].any() and not both[3, 1].any() and both[4, 0].any() and both[4, 1].any()      # 624 / 499: the intervals overlap at 499 only


def test_scale_table_refusals(pkg):
    for k, n, single, word in ((dict(scales=[1.0, 2.0, 3.0]), 2, False, "n_scales"), (dict(scale=float("nan")), 2, False, "finite"),
                               (dict(t_range=(5, 1)), 2, False, "interval"), (dict(), 5, False, "batch"), (dict(), 9, True, "batch"), (dict(), 0, False, "batch")):
        with pytest.raises(pkg.InvalidArgument, match=word):
            pkg.control_scale_table(pkg.make_control(**k), n, TS8, single_branch=single)
    out = pkg.control_scale_table(pkg.control_default(), 8, [], single_branch=True)      # no iteration: the sentinel row alone
    assert out.shape == (1, 8) and not out.any()
    assert pkg.lib().sdxl_control_scale_table(None, 2, 0, None, 0, None) != 0


# ---------------------------------------------------------------------------------------------------------------- the fixture
def cpu_noise(n, h, w):
    """the noise callable of cpu_controlled_loop from CPU generators: no GPU"""
    return lambda key: seeded(n, 4, h, w, seed=7 if key[0] == "initial" else 100 + key[1])


def test_fixture_matters_and_behaves():
    """Tiny configuration, 16 x 16 latent, n = 2, 4 DDIM steps at guidance 7.5, control seed 1 with the block hint of seed 1, conditioning scale 1.0 --
    the first one tried: the synthetic gain-1.5 hint convolutions do not make the trajectory grow, so nothing was lowered.  On this run:
      finite at every iteration (max |latent| per iteration 15.5, 33.9, 53.0, 65.7);
      max |controlled| = 65.74 against max |plain| = 61.18, a factor 1.07 (bound: 2);
      max |controlled - plain| = 40.44, against 100 x the f16 latent bar = 100 x 6e-3 x 65.74 = 39.44."""
    ocfg, n, steps = OC.tiny_config(), 2, 4
    W, Wc = unet_weights(ocfg), CR.control_weights(ocfg, 1)
    _, oc = _cond(ocfg, n, (128, 128))
    table = R.coefficients(ALPHAS, steps, 0, R.DDIM, 0.0)
    noise = cpu_noise(n, 16, 16)
    plain = TR.cpu_controlled_loop(ocfg, W, ALPHAS, oc, 7.5, steps, n, table, noise, [])
    trace = []
    ctl = [dict(W=Wc, hint=CR.block_hint(n, 128, 128, 1), options=dict(scale=CONTROL_SCALE))]
    out = TR.cpu_controlled_loop(ocfg, W, ALPHAS, oc, 7.5, steps, n, table, noise, ctl, trace=trace)
    assert len(trace) == steps and TR.first_non_finite(torch.stack(trace), n) is None
    top, base, moved = out.abs().max().item(), plain.abs().max().item(), (out - plain).abs().max().item()
    print(f"control seed 1 scale {CONTROL_SCALE}: max |controlled| {top:.2f}, max |plain| {base:.2f}, max |controlled - plain| {moved:.2f}, "
          f"100 x f16 bar {100 * LAT_REL_F16 * top:.2f}; per iteration {[round(x.abs().max().item(), 1) for x in trace]}")
    assert top <= 2.0 * base, "the control net makes the trajectory grow: lower CONTROL_SCALE"
    assert moved >= 100 * LAT_REL_F16 * top, "the control net does not matter: the trajectory bars would show nothing"
    # scale 0 and an interval without an iteration are the plain trajectory, bit for bit: no net is evaluated
    for options in (dict(scale=0.0), dict(t_range=(1000, 2000))):
        ctl[0]["options"] = options
        assert torch.equal(TR.cpu_controlled_loop(ocfg, W, ALPHAS, oc, 7.5, steps, n, table, noise, ctl), plain)
