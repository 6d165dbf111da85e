"""Noise-level schedules through the Diffuser: sigma lists, end levels, sdxl_continue_latent (the base -> refiner handoff) and DPM++ 3M SDE
against a CPU loop around the oracle's UNet fed float timesteps (tests/levels_ref.py cpu_loop), on the tiny nets, resolutions and conditioning
of tests/test_gpu_solver.py.

Bar of a trajectory: lat_tol(dtype, ref) of tests/test_gpu_models.py times G = max(1, g / g_DDIM), the rule tests/test_gpu_solver.py derives
and tests/test_gpu_fewstep.py reuses.  g is the first-order gain of a UNet-output error onto the latent, sum_i (|c_0,i| k_i + |c_1,i| k_{i-1} +
|c_2,i| k_{i-2}), k = sigma / alpha, of the case's fp64 table on its schedule (levels_ref.error_gain).  g_DDIM is solver_ref.error_gain of the
DDIM table on the default schedule, what lat_tol was set for; no default schedule has six entries (n_steps = 5 gives five, 6 gives seven), so
it is the larger of those two neighbours (4.78), the stricter bar."""
import ctypes

import numpy as np
import pytest
import torch

import levels_ref as L
import solver_ref as R
from oracle import config as OC, pipeline as OP
from test_gpu_models import _cond, _pkg_cond, lat_tol, weights_for
from test_gpu_solver import _inpaint_inputs
from util import max_abs, seeded, to_pkg_cfg

pytestmark = pytest.mark.gpu

ALPHAS = OC.alphas_cumprod()
K6, E6 = L.sigmas_karras(6, ALPHAS), L.sigmas_exponential(6, ALPHAS)
T6 = [999, 800, 600, 400, 200, 50]
SEEDS = [1234, 0xDEADBEEFCAFEF00D]
RES = (64, 96)
G_DDIM = max(R.error_gain(R.coefficients(ALPHAS, n, 0, R.DDIM, 0.0), ALPHAS, n, 0) for n in (5, 6))
_refs = {}


def _diffuser(pkg, ctx, ocfg, dtype, solver="ddim"):
    d = pkg.Diffuser(ctx, to_pkg_cfg(pkg, ocfg), dtype, seed=weights_for(pkg, ocfg, dtype)[1])
    d.set_solver(solver)
    return d


def _gain(table, lv):
    g = L.error_gain(table, lv)
    return max(1.0, g / G_DDIM), g


def _report(what, out, ref, dtype, G, g):
    tol = lat_tol(dtype, ref) * G
    e = max_abs(out, ref)
    print(f"levels {what} dtype={dtype}: latent max-abs err {e:.3e} (bar {tol:.3e}, ratio {e / tol:.3f}, G {G:.3f} from g {g:.2f} / g_DDIM {G_DDIM:.2f}, "
          f"|latent| max {ref.abs().max():.2f})")
    assert np.isfinite(e) and e < tol
    return tol


def _ref(key, make):
    """the CPU reference of a case, computed once: dtypes 0, 1 and 3 run the same weights"""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def _noise(pkg, ctx, seeds, h, w):
    return lambda draw: pkg.gen_noise(ctx, seeds, draw, len(seeds), h, w).cpu()


def _set(d, sched):
    """a schedule dict (sigmas / sigma_end / round_t, or timesteps / t_end) onto a handle"""
    if "sigmas" in sched:
        d.set_sigmas(sched["sigmas"], sched.get("sigma_end", 0.0), sched.get("round_t", False))
    else:
        d.set_timesteps(sched["timesteps"], sched.get("t_end", -1))


# ------------------------------------------------------------------------------------------------ sampling against the CPU loop

SAMPLING = [("dpmpp_2m", 0.0, "K6"), ("dpmpp_2m", 1.0, "K6"), ("dpmpp_3m", 0.0, "K6"), ("dpmpp_3m", 1.0, "K6"), ("ddim", 0.0, "E6"), ("dpmpp_2m", 0.0, "K6r")]
SCHEDS = {"K6": dict(sigmas=K6), "E6": dict(sigmas=E6), "K6r": dict(sigmas=K6, round_t=True)}


@pytest.mark.parametrize("dtype", [0, 1, 3])
@pytest.mark.parametrize("n,cfg_scale", [(1, 7.5), (2, 1.0)])
@pytest.mark.parametrize("solver,eta,sched", SAMPLING)
def test_sampling_against_cpu_loop(pkg, ctx, solver, eta, sched, n, cfg_scale, dtype):
    ocfg = OC.tiny_config()
    h, w = RES[0] // 8, RES[1] // 8
    c, oc = _cond(ocfg, n, RES)
    lv = L.levels(ALPHAS, **SCHEDS[sched])
    table = L.coefficients(lv, solver, eta)
    G, g = _gain(table, lv)
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ALPHAS)
    noise = _noise(pkg, ctx, SEEDS[:n], h, w)
    ref = _ref(("sample", solver, eta, sched, n), lambda: L.cpu_loop(od, oc, cfg_scale, lv, table, noise(pkg.DRAW_INITIAL), noise))
    d = _diffuser(pkg, ctx, ocfg, dtype, solver)
    _set(d, SCHEDS[sched])
    out = d.sample_latent(_pkg_cond(pkg, c, RES), cfg_scale, 6, seeds=SEEDS[:n], eta=eta).cpu()
    _report(f"sample {solver} eta={eta} n={n} {sched}", out, ref, dtype, G, g)


@pytest.mark.parametrize("dtype", [0, 3])
def test_3m_inpainting_against_cpu_loop(pkg, ctx, dtype):
    ocfg, res = OC.tiny_config(), (64, 64)
    c, oc = _cond(ocfg, 1, res)
    reference, mask = _inpaint_inputs()
    seeds = [4321]
    lv = L.levels(ALPHAS, sigmas=K6)
    table = L.coefficients(lv, "dpmpp_3m", 1.0)
    G, g = _gain(table, lv)
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ALPHAS)
    noise = _noise(pkg, ctx, seeds, 8, 8)
    ref = _ref("inpaint", lambda: L.cpu_loop(od, oc, 7.5, lv, table, noise(pkg.DRAW_INITIAL), noise, reference=reference, mask=mask))
    d = _diffuser(pkg, ctx, ocfg, dtype, "dpmpp_3m")
    d.set_sigmas(K6)
    out = d.sample_latent_with_inpainting(_pkg_cond(pkg, c, res), 7.5, 6, reference.cuda(), mask.cuda(), seeds=seeds, eta=1.0).cpu()
    _report("3m inpainting K6", out, ref, dtype, G, g)


# ------------------------------------------------------------------------------------------------ the handoff

def _split(sched):
    """a 6-entry schedule as its first four entries ending on the fifth, and its last two"""
    if "sigmas" in sched:
        s = sched["sigmas"]
        return dict(sigmas=s[:4], sigma_end=s[4]), dict(sigmas=s[4:])
    t = sched["timesteps"]
    return dict(timesteps=t[:4], t_end=t[4]), dict(timesteps=t[4:])


@pytest.mark.parametrize("dtype", [0, 1, 3])
@pytest.mark.parametrize("sched", [dict(timesteps=T6), dict(sigmas=K6)], ids=["timesteps", "sigmas"])
def test_ddim_handoff_is_bit_equal_to_the_whole_run(pkg, ctx, sched, dtype):
    ocfg, n = OC.tiny_config(), 2
    c, _ = _cond(ocfg, n, RES)
    pc = _pkg_cond(pkg, c, RES)
    noise0 = pkg.gen_noise(ctx, SEEDS, pkg.DRAW_INITIAL, n, RES[0] // 8, RES[1] // 8)
    d = _diffuser(pkg, ctx, ocfg, dtype)
    _set(d, sched)
    whole = d.sample_latent(pc, 7.5, 6, noise0)
    first, second = _split(sched)
    _set(d, first)
    part = d.sample_latent(pc, 7.5, 4, noise0)
    assert torch.isfinite(part).all() and not torch.equal(part, whole)
    _set(d, second)
    out = d.continue_latent(part, pc, 7.5, 2)
    assert torch.equal(out.view(torch.int32), whole.view(torch.int32)), "4 + 2 differs from the one 6-entry run"
    assert torch.equal(d.continue_latent(part, pc, 7.5, 2, seeds=SEEDS), whole), "eta = 0 draws nothing: seeds change no bit"


@pytest.mark.parametrize("dtype", [0, 1, 3])
@pytest.mark.parametrize("solver,eta", [("dpmpp_2m", 0.0), ("dpmpp_3m", 1.0)])
def test_multistep_handoff_restarts_the_order(pkg, ctx, solver, eta, dtype):
    ocfg, n = OC.tiny_config(), 2
    h, w = RES[0] // 8, RES[1] // 8
    c, oc = _cond(ocfg, n, RES)
    pc = _pkg_cond(pkg, c, RES)
    first, second = _split(dict(sigmas=K6))
    lv1, lv2 = L.levels(ALPHAS, **first), L.levels(ALPHAS, **second)
    t1, t2 = L.coefficients(lv1, solver, eta), L.coefficients(lv2, solver, eta)
    assert t2[0][2] == 0.0 and t2[0][3] == 0.0, "the continued piece starts first order"
    G, g = _gain(np.concatenate([t1, t2]), lv1 + lv2)
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ALPHAS)
    noise = _noise(pkg, ctx, SEEDS, h, w)
    ref = _ref(("split", solver), lambda: L.cpu_loop(od, oc, 7.5, lv2, t2, L.cpu_loop(od, oc, 7.5, lv1, t1, noise(pkg.DRAW_INITIAL), noise), noise))
    d = _diffuser(pkg, ctx, ocfg, dtype, solver)
    _set(d, first)
    part = d.sample_latent(pc, 7.5, 4, seeds=SEEDS, eta=eta)
    _set(d, second)
    out = d.continue_latent(part, pc, 7.5, 2, seeds=SEEDS, eta=eta).cpu()
    _report(f"handoff {solver} eta={eta} 4 + 2 of K6", out, ref, dtype, G, g)


@pytest.mark.parametrize("dtype", [0, 3])
def test_base_to_refiner_handoff(pkg, ctx, dtype):
    """the base handle stops at sigma K6[4], the refiner handle continues from that latent without re-noising: against a CPU loop that switches weights"""
    bcfg, rcfg, n, res = OC.tiny_config(), OC.tiny_refiner_config(), 1, (64, 64)
    cb, ocb = _cond(bcfg, n, res)
    cr, ocr = _cond(rcfg, n, res, refiner=True)
    seeds = [77]
    first, second = _split(dict(sigmas=K6))
    lv1, lv2 = L.levels(ALPHAS, **first), L.levels(ALPHAS, **second)
    t1, t2 = L.coefficients(lv1, "dpmpp_2m", 0.0), L.coefficients(lv2, "dpmpp_2m", 0.0)
    G, g = _gain(np.concatenate([t1, t2]), lv1 + lv2)
    odb = OP.Diffuser(bcfg, weights_for(pkg, bcfg, dtype)[0], ALPHAS)
    odr = OP.Diffuser(rcfg, weights_for(pkg, rcfg, dtype)[0], ALPHAS)
    noise = _noise(pkg, ctx, seeds, 8, 8)
    ref = _ref("refiner", lambda: L.cpu_loop(odr, ocr, 7.5, lv2, t2, L.cpu_loop(odb, ocb, 7.5, lv1, t1, noise(pkg.DRAW_INITIAL), noise), noise, refiner=True))
    base, refiner = _diffuser(pkg, ctx, bcfg, dtype, "dpmpp_2m"), _diffuser(pkg, ctx, rcfg, dtype, "dpmpp_2m")
    _set(base, first)
    _set(refiner, second)
    part = base.sample_latent(_pkg_cond(pkg, cb, res), 7.5, 4, seeds=seeds)
    out = refiner.continue_latent(part, _pkg_cond(pkg, cr, res, True), 7.5, 2).cpu()
    _report("base -> refiner 4 + 2 of K6", out, ref, dtype, G, g)


@pytest.mark.parametrize("dtype", [0, 1, 3])
def test_continue_with_renoise_against_cpu_loop(pkg, ctx, dtype):
    ocfg, n = OC.tiny_config(), 2
    h, w = RES[0] // 8, RES[1] // 8
    c, oc = _cond(ocfg, n, RES)
    pc = _pkg_cond(pkg, c, RES)
    latent = seeded(n, 4, h, w, seed=41)
    sg = K6[2:]
    lv = L.levels(ALPHAS, sigmas=sg)
    table = L.coefficients(lv, "dpmpp_3m", 0.0)
    G, g = _gain(table, lv)
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ALPHAS)
    noise = _noise(pkg, ctx, SEEDS, h, w)
    a0 = lv[0][1]
    ref = _ref("renoise", lambda: L.cpu_loop(od, oc, 7.5, lv, table, latent * (a0 ** 0.5) + noise(pkg.DRAW_INITIAL) * ((1.0 - a0) ** 0.5), noise))
    d = _diffuser(pkg, ctx, ocfg, dtype, "dpmpp_3m")
    d.set_sigmas(sg)
    out = d.continue_latent(latent.cuda(), pc, 7.5, 4, seeds=SEEDS, renoise=True)
    tol = _report("continue renoise 3m K6[2:]", out.cpu(), ref, dtype, G, g)
    explicit = d.continue_latent(latent.cuda(), pc, 7.5, 4, noise=pkg.gen_noise(ctx, SEEDS, pkg.DRAW_INITIAL, n, h, w), renoise=True)
    assert torch.equal(explicit, out), "the explicit tensor of the same draw gives other bits"
    assert max_abs(d.continue_latent(latent.cuda(), pc, 7.5, 4).cpu(), out.cpu()) > tol, "renoise is not live"


# ------------------------------------------------------------------------------------------------ liveness, defaults, stale state

@pytest.mark.parametrize("dtype", [0, 1, 3])
def test_sigma_list_end_level_and_solver_are_live(pkg, ctx, dtype):
    ocfg, n = OC.tiny_config(), 2
    c, _ = _cond(ocfg, n, RES)
    pc = _pkg_cond(pkg, c, RES)
    d = _diffuser(pkg, ctx, ocfg, dtype, "dpmpp_2m")
    run = lambda: d.sample_latent(pc, 7.5, 4, seeds=SEEDS).cpu()
    default = run()
    d.set_sigmas(K6[:4])
    karras = run()
    d.set_sigmas(K6[:4], sigma_end=K6[4])      # the latent at sigma 0.17, not the data
    ended = run()
    d.set_sigmas(K6[:4], round_t=True)
    rounded = run()
    d.set_sigmas(K6[:4])
    d.set_solver("dpmpp_3m")
    third = run()
    lv = L.levels(ALPHAS, sigmas=K6[:4])
    tol = lat_tol(dtype, karras) * max(_gain(L.coefficients(lv, s, 0.0), lv)[0] for s in ("dpmpp_2m", "dpmpp_3m"))
    print(f"levels liveness dtype={dtype}: sigmas against default {max_abs(karras, default):.3e}, end level {max_abs(ended, karras):.3e}, "
          f"3M against 2M {max_abs(third, karras):.3e}, ROUND_T {max_abs(rounded, karras):.3e} (bar {tol:.3e})")
    assert max_abs(karras, default) > tol, "the sigma list is not live"
    assert max_abs(ended, karras) > tol, "the end level is not live"
    assert max_abs(third, karras) > tol, "the 3M rows are not live"
    assert not torch.equal(rounded, karras), "ROUND_T changes the timestep the UNet is fed"


@pytest.mark.parametrize("dtype", [0, 1])
def test_default_bits_survive_a_round_trip(pkg, ctx, dtype):
    ocfg = OC.tiny_config()
    c, _ = _cond(ocfg, 2, RES)
    pc = _pkg_cond(pkg, c, RES)
    seeds = [9, 10]
    noise0 = pkg.gen_noise(ctx, seeds, pkg.DRAW_INITIAL, 2, 8, 12)
    d = pkg.Diffuser(ctx, to_pkg_cfg(pkg, ocfg), dtype, seed=weights_for(pkg, ocfg, dtype)[1])
    assert d.sigmas is None and d.timesteps is None and d.timesteps_end == -1 and d.solver == "ddim"
    first = d.sample_latent(pc, 7.5, 4, seeds=seeds, eta=0.5)
    first_explicit = d.sample_latent(pc, 7.5, 4, noise0)
    d.set_timesteps([999, 759, 499, 259])
    listed = d.sample_latent(pc, 7.5, 4, noise0)
    d.set_sigmas(K6, sigma_end=0.01, round_t=True)
    d.set_solver("dpmpp_3m")
    assert d.sigmas == (K6, 0.01, True) and d.timesteps is None and d.solver == "dpmpp_3m", "while a sigma list is set it is the list in force"
    other = d.sample_latent(pc, 7.5, 6, seeds=seeds, eta=1.0)
    assert torch.isfinite(other).all()
    for bad in ([1.0, 2.0], [2.0, 2.0], [2.0, 0.0], [float("nan")]):
        with pytest.raises(pkg.InvalidArgument, match="sigmas"):
            d.set_sigmas(bad)
    with pytest.raises(pkg.InvalidArgument, match="sigmas"):
        d.set_sigmas(K6, sigma_end=K6[-1])
    assert d.sigmas == (K6, 0.01, True), "a refused list replaced the handle's"
    d.set_sigmas(None)
    d.set_solver("ddim")
    assert d.sigmas is None and d.timesteps == [999, 759, 499, 259], "back on the timestep list the handle had before"
    assert torch.equal(d.sample_latent(pc, 7.5, 4, noise0), listed)
    d.set_timesteps([999, 759, 499, 259], t_end=100)
    assert d.timesteps_end == 100 and not torch.equal(d.sample_latent(pc, 7.5, 4, noise0), listed)
    with pytest.raises(pkg.InvalidArgument, match="timesteps"):
        d.set_timesteps([999, 759, 499, 259], t_end=259)
    assert d.timesteps_end == 100
    d.set_sigmas(K6)
    d.set_timesteps(None)
    assert d.sigmas is None and d.timesteps is None and d.timesteps_end == -1, "setting (or clearing) a timestep list drops the sigma list"
    assert torch.equal(d.sample_latent(pc, 7.5, 4, seeds=seeds, eta=0.5), first)
    assert torch.equal(d.sample_latent(pc, 7.5, 4, noise0), first_explicit)
    fresh = pkg.Diffuser(ctx, to_pkg_cfg(pkg, ocfg), dtype, seed=weights_for(pkg, ocfg, dtype)[1])
    assert torch.equal(fresh.sample_latent(pc, 7.5, 4, seeds=seeds, eta=0.5), first)


@pytest.mark.parametrize("dtype", [0, 1])
def test_second_history_is_not_stale(pkg, ctx, dtype):
    """two 3M calls in a row at different resolutions, batch sizes and lengths: the second equals a fresh handle's"""
    ocfg = OC.tiny_config()
    c2, _ = _cond(ocfg, 2, RES)
    c1, _ = _cond(ocfg, 1, (64, 64))
    d = _diffuser(pkg, ctx, ocfg, dtype, "dpmpp_3m")
    d.set_sigmas(K6)
    big = d.sample_latent(_pkg_cond(pkg, c2, RES), 7.5, 6, seeds=SEEDS, eta=1.0)
    d.set_sigmas(E6[:4])
    small = d.sample_latent(_pkg_cond(pkg, c1, (64, 64)), 7.5, 4, seeds=[5], eta=1.0)
    again = d.sample_latent(_pkg_cond(pkg, c2, RES), 7.5, 4, seeds=SEEDS, eta=1.0)
    fresh = _diffuser(pkg, ctx, ocfg, dtype, "dpmpp_3m")
    fresh.set_sigmas(E6[:4])
    assert torch.isfinite(big).all() and torch.isfinite(small).all()
    assert torch.equal(fresh.sample_latent(_pkg_cond(pkg, c1, (64, 64)), 7.5, 4, seeds=[5], eta=1.0), small)
    assert torch.equal(fresh.sample_latent(_pkg_cond(pkg, c2, RES), 7.5, 4, seeds=SEEDS, eta=1.0), again)


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_launch_nothing(pkg, ctx):
    ocfg, res = OC.tiny_config(), (64, 64)
    c, _ = _cond(ocfg, 1, res)
    pc = _pkg_cond(pkg, c, res)
    d = _diffuser(pkg, ctx, ocfg, 0)
    l = pkg.lib()
    cc, keep = pc.to_c()
    out = torch.full((1, 4, 8, 8), 7.25, device="cuda")
    latent = pkg.gen_noise(ctx, [5], pkg.DRAW_INITIAL, 1, 8, 8)
    seeds = (ctypes.c_uint64 * 1)(5)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    dbl = ctypes.c_double

    def cont(n_steps=6, noise=None, seeded=False, eta=0.0, renoise=0):
        return l.sdxl_continue_latent(d.h, None, p(latent), ctypes.byref(cc), dbl(7.5), n_steps, p(noise), seeds if seeded else None, dbl(eta), renoise, p(out))

    def refused(call, word):
        rc = call()
        torch.cuda.synchronize()
        msg = l.sdxl_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)
        assert bool((out == 7.25).all()), "the output was written"

    refused(cont, "list")                                                     # a handle without a list
    d.set_sigmas(K6)
    refused(lambda: cont(n_steps=5), "sigmas")                                # n_steps differs from the list's length
    refused(lambda: cont(renoise=1), "exactly one")                           # renoise without noise
    refused(lambda: cont(renoise=1, noise=latent, seeded=True), "exactly one")
    refused(lambda: cont(eta=0.5), "seeds")                                   # eta without seeds
    refused(lambda: cont(eta=1.5, seeded=True), "eta")
    refused(lambda: l.sdxl_refine_latent_seeded(d.h, None, p(latent), ctypes.byref(cc), dbl(7.5), 800, 6, seeds, dbl(0.0), p(out)), "sdxl_continue_latent")
    refused(lambda: l.sdxl_refine_latent(d.h, None, p(latent), ctypes.byref(cc), dbl(7.5), 800, 6, p(latent), p(out)), "sdxl_continue_latent")
    refused(lambda: l.sdxl_sample_latent_seeded(d.h, None, ctypes.byref(cc), dbl(7.5), 5, seeds, dbl(0.0), p(out)), "sigmas")
    d.set_solver("tcd")
    refused(lambda: l.sdxl_sample_latent_seeded(d.h, None, ctypes.byref(cc), dbl(7.5), 6, seeds, dbl(0.3), p(out)), "sigmas")   # TCD on a sigma list
    refused(lambda: cont(seeded=True, eta=0.3), "sigmas")
    d.set_solver("lcm")
    refused(cont, "seeded")                                                   # c_z != 0 and no seeds
    d.set_solver("dpmpp_3m")
    assert d.sigmas == (K6, 0.0, False) and d.solver == "dpmpp_3m", "a refusal changed the handle"
    assert cont() == 0, l.sdxl_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not bool((out == 7.25).any())
    for unknown in (2, 7, -1):
        with pytest.raises(pkg.EngineError, match="solver"):
            d.set_solver(unknown)
    assert d.solver == "dpmpp_3m"
