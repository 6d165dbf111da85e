"""Few-step sampling through the Diffuser: timestep lists (sdxl_diffuser_set_timesteps) and the LCM / TCD solvers against a CPU loop around
the oracle (tests/fewstep_ref.py cpu_loop), on the tiny nets, resolutions and conditioning of tests/test_gpu_solver.py.

Bar of a trajectory: lat_tol(dtype, ref) of tests/test_gpu_models.py times G = max(1, g / g_DDIM).  g is the first-order gain of a
UNet-output error onto the latent, sum_i |c_0,i| sigma_i / alpha_i (+ the c_1 term under 2M; sigma_i alone under v-prediction, where x0
carries no 1 / alpha), of the case's fp64 table on its list; g_DDIM is solver_ref.error_gain of the DDIM table on the default schedule of the
same length, what lat_tol was set for.  The rule is the one tests/test_gpu_solver.py derives and tests/test_gpu_prediction.py reuses."""
import numpy as np
import pytest
import torch

import fewstep_ref as F
import prediction_ref as P
import solver_ref as R
from oracle import config as OC, pipeline as OP
from test_gpu_models import _cond, _pkg_cond, lat_tol, weights_for
from test_gpu_solver import _inpaint_inputs
from util import max_abs, seeded, to_pkg_cfg

pytestmark = pytest.mark.gpu

ALPHAS = OC.alphas_cumprod()
ZT = P.rescale_zero_terminal_snr(ALPHAS)[1]
L4, L5, UNEVEN, REFINE = F.schedule_lcm(4), F.schedule_lcm(5), [900, 650, 300, 20], [199, 139, 79, 19]
SEEDS = [1234, 0xDEADBEEFCAFEF00D]
RES = (64, 96)
_refs = {}


def _diffuser(pkg, ctx, ocfg, dtype, solver="ddim", ts=None, alphas=None, prediction="epsilon"):
    d = pkg.Diffuser(ctx, to_pkg_cfg(pkg, ocfg), dtype, seed=weights_for(pkg, ocfg, dtype)[1], alphas_cumprod=alphas)
    d.set_solver(solver)
    d.set_timesteps(ts)
    d.set_prediction(prediction)
    return d


def _table(alphas, ts, solver, eta, prediction="epsilon", default=None):
    """(the fp64 table the trajectory runs, G, g, g_DDIM); default: (n_steps, step_start) of the default schedule of the list's length"""
    n_steps, step_start = default if default is not None else (len(ts), 0)
    assert len(R.schedule(ALPHAS, n_steps, step_start)) == len(ts)
    table = F.coefficients(alphas, ts, solver, eta)
    g = F.error_gain(table, alphas, ts, prediction)
    g_ddim = R.error_gain(R.coefficients(ALPHAS, n_steps, step_start, R.DDIM, 0.0), ALPHAS, n_steps, step_start)
    return table, max(1.0, g / g_ddim), g, g_ddim


def _report(what, out, ref, dtype, G, g, g_ddim):
    tol = lat_tol(dtype, ref) * G
    e = max_abs(out, ref)
    print(f"fewstep {what} dtype={dtype}: latent max-abs err {e:.3e} (bar {tol:.3e}, G {G:.3f} from g {g:.2f} / g_DDIM {g_ddim:.2f}, |latent| max {ref.abs().max():.2f})")
    assert np.isfinite(e) and e < tol
    return tol


def _ref(key, make):
    """the CPU reference of a case, computed once: dtypes 0, 1 and 3 run the same weights"""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


# ------------------------------------------------------------------------------------------------ sampling against the CPU loop

SAMPLING = [("lcm", 0.0), ("tcd", 0.3), ("tcd", 1.0)]


@pytest.mark.parametrize("dtype", [0, 1, 3])
@pytest.mark.parametrize("n,cfg_scale", [(1, 7.5), (2, 1.0)])
@pytest.mark.parametrize("solver,gamma", SAMPLING)
def test_sampling_against_cpu_loop(pkg, ctx, solver, gamma, n, cfg_scale, dtype):
    ocfg = OC.tiny_config()
    h, w = RES[0] // 8, RES[1] // 8
    c, oc = _cond(ocfg, n, RES)
    table, G, g, g_ddim = _table(ALPHAS, L4, solver, gamma)
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ALPHAS)
    ref = _ref(("sample", solver, gamma, n), lambda: F.cpu_loop(od, pkg, ctx, oc, cfg_scale, L4, table, "epsilon", SEEDS[:n], h, w))
    d = _diffuser(pkg, ctx, ocfg, dtype, solver, L4)
    out = d.sample_latent(_pkg_cond(pkg, c, RES), cfg_scale, len(L4), seeds=SEEDS[:n], eta=gamma).cpu()
    _report(f"sample {solver} gamma={gamma} n={n} list={L4}", out, ref, dtype, G, g, g_ddim)


@pytest.mark.parametrize("dtype", [0, 1, 3])
@pytest.mark.parametrize("mode", ["off", "cfg1.5"])
def test_lcm_guidance_forms(pkg, ctx, mode, dtype):
    """LCM-LoRA is run without guidance and with a scale near 1"""
    ocfg, n = OC.tiny_config(), 2
    h, w = RES[0] // 8, RES[1] // 8
    c, oc = _cond(ocfg, n, RES)
    table, G, g, g_ddim = _table(ALPHAS, L4, "lcm", 0.0)
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ALPHAS)
    ref = _ref(("guidance", mode), lambda: F.cpu_loop(od, pkg, ctx, oc, 1.5, L4, table, "epsilon", SEEDS, h, w, off=mode == "off"))
    d = _diffuser(pkg, ctx, ocfg, dtype, "lcm", L4)
    if mode == "off":
        d.set_guidance(mode="off")
        pc = pkg.Conditioning(context_full=c["ctx"].cuda(), channel_context=c["y"].cuda(), resolution=RES)
    else:
        pc = _pkg_cond(pkg, c, RES)
    out = d.sample_latent(pc, 1.5, 4, seeds=SEEDS).cpu()
    _report(f"lcm guidance {mode}", out, ref, dtype, G, g, g_ddim)


@pytest.mark.parametrize("dtype", [0, 1, 3])
@pytest.mark.parametrize("solver,eta", [("ddim", 0.5), ("dpmpp_2m", 0.0)])
def test_old_solvers_on_an_uneven_list(pkg, ctx, solver, eta, dtype):
    """lists are live for DDIM and 2M: the trajectory follows the list's (a, ap), and differs from the default schedule of the same length"""
    ocfg, n = OC.tiny_config(), 2
    h, w = RES[0] // 8, RES[1] // 8
    c, oc = _cond(ocfg, n, RES)
    table, G, g, g_ddim = _table(ALPHAS, UNEVEN, solver, eta)
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ALPHAS)
    ref = _ref(("uneven", solver), lambda: F.cpu_loop(od, pkg, ctx, oc, 7.5, UNEVEN, table, "epsilon", SEEDS, h, w))
    d = _diffuser(pkg, ctx, ocfg, dtype, solver, UNEVEN)
    pc = _pkg_cond(pkg, c, RES)
    out = d.sample_latent(pc, 7.5, 4, seeds=SEEDS, eta=eta).cpu()
    tol = _report(f"{solver} eta={eta} list={UNEVEN}", out, ref, dtype, G, g, g_ddim)
    d.set_timesteps(None)
    assert max_abs(d.sample_latent(pc, 7.5, 4, seeds=SEEDS, eta=eta).cpu(), out) > tol, "the list is not live"


@pytest.mark.parametrize("dtype", [0, 3])
def test_lcm_inpainting_against_cpu_loop(pkg, ctx, dtype):
    ocfg, res = OC.tiny_config(), (64, 64)
    c, oc = _cond(ocfg, 1, res)
    reference, mask = _inpaint_inputs()
    seeds = [4321]
    table, G, g, g_ddim = _table(ALPHAS, L5, "lcm", 0.0)
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ALPHAS)
    ref = _ref("inpaint", lambda: F.cpu_loop(od, pkg, ctx, oc, 7.5, L5, table, "epsilon", seeds, 8, 8, reference, mask))
    d = _diffuser(pkg, ctx, ocfg, dtype, "lcm", L5)
    out = d.sample_latent_with_inpainting(_pkg_cond(pkg, c, res), 7.5, 5, reference.cuda(), mask.cuda(), seeds=seeds).cpu()
    _report(f"lcm inpainting list={L5}", out, ref, dtype, G, g, g_ddim)


@pytest.mark.parametrize("dtype", [0, 3])
def test_tcd_refine_against_cpu_loop(pkg, ctx, dtype):
    """a refiner handle, step_start 800: the re-noise level is alphas[200] and the list starts at 199, the reference's own relation"""
    ocfg, res, step_start, gamma = OC.tiny_refiner_config(), (64, 64), 800, 0.3
    c, oc = _cond(ocfg, 1, res, refiner=True)
    latent = seeded(1, 4, 8, 8, seed=41)
    seeds = [77]
    table, G, g, g_ddim = _table(ALPHAS, REFINE, "tcd", gamma, default=(20, 800))
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ALPHAS)
    ref = _ref("refine", lambda: F.cpu_loop(od, pkg, ctx, oc, 7.5, REFINE, table, "epsilon", seeds, 8, 8, latent0=latent, renoise_t=1000 - step_start))
    d = _diffuser(pkg, ctx, ocfg, dtype, "tcd", REFINE)
    pc = _pkg_cond(pkg, c, res, True)
    out = d.refine_latent(latent.cuda(), pc, 7.5, step_start, 4, seeds=seeds, eta=gamma).cpu()
    _report(f"tcd refine gamma={gamma} list={REFINE}", out, ref, dtype, G, g, g_ddim)
    d.set_timesteps([179, 139, 79, 19])
    with pytest.raises(pkg.InvalidArgument, match="timesteps"):
        d.refine_latent(latent.cuda(), pc, 7.5, step_start, 4, seeds=seeds, eta=gamma)
    d.set_timesteps(REFINE)
    with pytest.raises(pkg.InvalidArgument, match="timesteps"):
        d.refine_latent(latent.cuda(), pc, 7.5, step_start, 10, seeds=seeds, eta=gamma)
    assert torch.equal(d.refine_latent(latent.cuda(), pc, 7.5, step_start, 4, seeds=seeds, eta=gamma).cpu(), out)


@pytest.mark.parametrize("dtype", [0, 1, 3])
def test_lcm_v_prediction_from_zero_terminal_snr(pkg, ctx, dtype):
    ocfg, n = OC.tiny_config(), 2
    h, w = RES[0] // 8, RES[1] // 8
    c, oc = _cond(ocfg, n, RES)
    assert L4[0] == 999 and ZT[999] == 0.0
    table, G, g, g_ddim = _table(ZT, L4, "lcm", 0.0, "v")
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ZT)
    ref = _ref("v", lambda: F.cpu_loop(od, pkg, ctx, oc, 7.5, L4, table, "v", SEEDS, h, w))
    d = _diffuser(pkg, ctx, ocfg, dtype, "lcm", L4, ZT, "v")
    out = d.sample_latent(_pkg_cond(pkg, c, RES), 7.5, 4, seeds=SEEDS).cpu()
    _report("lcm v-prediction zero-terminal", out, ref, dtype, G, g, g_ddim)


# ------------------------------------------------------------------------------------------------ liveness

@pytest.mark.parametrize("dtype", [0, 1, 3])
def test_solvers_gamma_and_seeds_are_live(pkg, ctx, dtype):
    ocfg, n = OC.tiny_config(), 2
    c, _ = _cond(ocfg, n, RES)
    pc = _pkg_cond(pkg, c, RES)
    d = _diffuser(pkg, ctx, ocfg, dtype, "lcm", L4)
    lcm = d.sample_latent(pc, 1.5, 4, seeds=SEEDS).cpu()
    other_seeds = d.sample_latent(pc, 1.5, 4, seeds=[5, 6]).cpu()
    d.set_solver("ddim")
    ddim = d.sample_latent(pc, 1.5, 4, seeds=SEEDS).cpu()
    d.set_solver("tcd")
    tcd0 = d.sample_latent(pc, 1.5, 4, seeds=SEEDS, eta=0.0).cpu()
    tcd1 = d.sample_latent(pc, 1.5, 4, seeds=SEEDS, eta=1.0).cpu()
    tol = lat_tol(dtype, lcm) * max(_table(ALPHAS, L4, "lcm", 0.0)[1], _table(ALPHAS, L4, "tcd", 1.0)[1])
    print(f"fewstep liveness dtype={dtype}: LCM against DDIM {max_abs(lcm, ddim):.3e}, TCD gamma 1 against 0 {max_abs(tcd1, tcd0):.3e}, "
          f"two seeds under LCM {max_abs(lcm, other_seeds):.3e} (bar {tol:.3e})")
    assert max_abs(lcm, ddim) > tol, "the LCM rows are not live"
    assert max_abs(tcd1, tcd0) > tol, "gamma is not live"
    assert max_abs(lcm, other_seeds) > tol, "the seeds are not live"


# ------------------------------------------------------------------------------------------------ the default is untouched

@pytest.mark.parametrize("dtype", [0, 1])
def test_default_bits_survive_a_round_trip(pkg, ctx, dtype):
    ocfg = OC.tiny_config()
    c, _ = _cond(ocfg, 2, RES)
    pc = _pkg_cond(pkg, c, RES)
    seeds = [9, 10]
    noise0 = pkg.gen_noise(ctx, seeds, pkg.DRAW_INITIAL, 2, 8, 12)
    d = pkg.Diffuser(ctx, to_pkg_cfg(pkg, ocfg), dtype, seed=weights_for(pkg, ocfg, dtype)[1])
    assert d.timesteps is None and d.solver == "ddim"
    first = d.sample_latent(pc, 7.5, 4, seeds=seeds, eta=0.5)
    first_explicit = d.sample_latent(pc, 7.5, 4, noise0)
    d.set_timesteps(L4)
    d.set_solver("lcm")
    assert d.timesteps == L4 and d.solver == "lcm"
    other = d.sample_latent(pc, 7.5, 4, seeds=seeds)
    assert torch.isfinite(other).all() and not torch.equal(other, first)
    with pytest.raises(pkg.InvalidArgument, match="timesteps"):
        d.set_timesteps([259, 499])
    with pytest.raises(pkg.InvalidArgument, match="timesteps"):
        d.set_timesteps([1000, 3])
    assert d.timesteps == L4, "a refused list replaced the handle's"
    d.set_solver("tcd")
    assert d.solver == "tcd"
    d.set_timesteps(None)
    d.set_solver("ddim")
    assert d.timesteps is None and d.solver == "ddim"
    assert torch.equal(d.sample_latent(pc, 7.5, 4, seeds=seeds, eta=0.5), first)
    assert torch.equal(d.sample_latent(pc, 7.5, 4, noise0), first_explicit)
    ts = pkg.timestep_schedule("reference", 4)
    d.set_timesteps(ts)
    assert d.timesteps == ts == [999, 749, 499, 249]
    assert torch.equal(d.sample_latent(pc, 7.5, 4, seeds=seeds, eta=0.5), first), "the reference's list gives other bits than the reference's rule"
    assert torch.equal(d.sample_latent(pc, 7.5, 4, noise0), first_explicit)
    d.set_timesteps([7])
    assert d.timesteps == [7]
    d.set_timesteps([])
    assert d.timesteps is None


# ------------------------------------------------------------------------------------------------ trace, timing, the guidance interval

@pytest.mark.parametrize("dtype", [0, 1])
def test_trace_timing_and_interval_read_the_list(pkg, ctx, dtype):
    ocfg, n = OC.tiny_config(), 2
    h, w = RES[0] // 8, RES[1] // 8
    c, oc = _cond(ocfg, n, RES)
    pc = _pkg_cond(pkg, c, RES)
    d = _diffuser(pkg, ctx, ocfg, dtype, "lcm", L4)
    plain = d.sample_latent(pc, 7.5, 4, seeds=SEEDS).cpu()
    trace = torch.zeros(6, n, 4, h, w, device="cuda")
    d.enable_step_timing(True)
    d.set_trace(trace)
    try:
        timed = d.sample_latent(pc, 7.5, 4, seeds=SEEDS).cpu()
        ms = d.step_times_ms()
    finally:
        d.set_trace(None)
        d.enable_step_timing(False)
    assert len(ms) == 4 and all(m > 0 for m in ms), "one timing record per list entry"
    assert torch.equal(timed, plain) and torch.equal(trace[3].cpu(), plain)
    assert all(float(trace[i].abs().max()) > 0 for i in range(4)) and not trace[4:].any(), "one trace record per list entry"
    # (400, 800) on 999, 759, 499, 259: the iterations at 999 and 259 run e = ec
    d.set_guidance(t_range=(400, 800))
    out = d.sample_latent(pc, 7.5, 4, seeds=SEEDS).cpu()
    table, G, g, g_ddim = _table(ALPHAS, L4, "lcm", 0.0)
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ALPHAS)
    ref = _ref("interval", lambda: F.cpu_loop(od, pkg, ctx, oc, 7.5, L4, table, "epsilon", SEEDS, h, w, t_range=(400, 800)))
    tol = _report("lcm interval (400, 800)", out, ref, dtype, G, g, g_ddim)
    assert max_abs(out, plain) > tol, "the interval is not live"
