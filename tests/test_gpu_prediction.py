"""v-prediction and zero-terminal-SNR schedules on the device: the v instantiations of the per-step kernel against the fp64 replay of
tests/prediction_ref.py (through sdxl_sampler_step_replay_pred), the handle option, the refusals, and whole trajectories against a CPU
loop around the oracle with its output read as v.

Bound of the kernel tests: for every recorded latent i, max|got - ref| <= 2^-24 * 8 * (i + 1) * M, M the largest value over the fp64
trajectory so far of |c_x x| + |c_0 x0| + |c_1 x0p| + |c_z z| (DDIM: |sqrt_ap x0| + |sqrt_1map e| + |sigma_t z|).  An update has at most
eight roundings that matter, each at most half an ulp of a term no larger than M, and the map x -> x' does not expand for these rows.
In front of latent 0 the only arithmetic is the step-0 inpainting blend, so there M is the size of its two terms (0 without inpainting:
latent 0 is the input, bit for bit).  An fp32 numpy emulation of the arithmetic stays below 0.3 of the bound: it is a condition, not a
measurement.

Bar of a whole trajectory: lat_tol(dtype, ref) of tests/test_gpu_models.py times G = max(1, g_v / g_eps_DDIM).  g_v = sum_i (|c_0,i| sigma_i
+ |c_1,i| sigma_{i-1}) is the first-order gain of a UNet-output error onto the latent under v (x0 = alpha x - sigma v: no 1 / alpha), from
the fp64 eta = 0 table of the solver on the zero-terminal schedule; g_eps_DDIM is solver_ref.error_gain of the epsilon DDIM table on the
default schedule, what lat_tol was set for.  The derivation is the one tests/test_gpu_solver.py states for its own G."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import prediction_ref as P
import solver_ref as R
from oracle import config as OC, pipeline as OP
from test_gpu_models import _cond, _pkg_cond, lat_tol, weights_for
from test_gpu_solver import _inpaint_inputs
from util import max_abs, seeded, to_pkg_cfg

pytestmark = pytest.mark.gpu

ALPHAS = OC.alphas_cumprod()
ZT = P.rescale_zero_terminal_snr(ALPHAS)[1]
N, H, W = 2, 8, 17            # HW = 136: the entry boundary falls inside a wave, two blocks with a ragged tail
HW = H * W
SEEDS = [1234, 0xDEADBEEFCAFEF00D]
SCALES = [3.0, 9.5]
MAX_ITERS = 8

# (noise, zero-terminal table, n_steps, guidance, inpainting, input_f16) -- every value of every column at least once, for both solvers.
# noise: None = explicit, else the eta of a seeded run.  guidance: "scalar" 7.5; "single" one branch; "rescale" per-entry scales with
# rescale = 0.7; "opts" the same within t_range = (300, 800)
ROWS = [
    (None, True, 4, "scalar", False, False), (None, False, 8, "single", True, True), (None, True, 8, "opts", True, False),
    (None, False, 4, "rescale", False, True), (0.0, True, 4, "opts", True, True), (0.0, False, 8, "scalar", False, False),
    (0.5, True, 8, "scalar", True, False), (0.5, False, 4, "opts", False, False), (0.5, True, 4, "single", False, True),
    (1.0, True, 8, "rescale", False, False), (1.0, False, 4, "single", True, False), (1.0, True, 4, "scalar", True, True),
    (1.0, True, 8, "opts", False, True),
]
CASES = [(solver,) + row for solver in ("ddim", "dpmpp_2m") for row in ROWS]


def _case_id(c):
    solver, eta, zt, n_steps, guidance, inpaint, f16 = c
    return "-".join([solver, "explicit" if eta is None else f"eta{eta}", "zt" if zt else "default", f"{n_steps}steps", guidance,
                     "inpaint" if inpaint else "plain", "f16in" if f16 else "f32in"])


@functools.lru_cache(maxsize=None)
def _inputs():
    """seeded normal v rows for the longest case and both branches, latent, reference, per-step noise; a mask with some rows kept"""
    mask = torch.zeros(N, 4, H, W, dtype=torch.bool)
    mask[:, :, 0:3, :] = True
    return dict(v=seeded(MAX_ITERS, 2 * N, HW, 4, seed=71), latent0=seeded(N, 4, H, W, seed=72), reference=seeded(N, 4, H, W, seed=73),
                step_noise=seeded(MAX_ITERS, N, 4, H, W, seed=74), mask=mask)


def _guidance(pkg, kind):
    """(Guidance or None, single, per-entry scales, rescale, t_range)"""
    if kind == "scalar":
        return None, False, [7.5] * N, 0.0, None
    if kind == "single":
        return None, True, None, 0.0, None
    if kind == "rescale":
        return pkg.make_guidance(scales=SCALES, rescale=0.7), False, SCALES, 0.7, None
    return pkg.make_guidance(scales=SCALES, rescale=0.7, t_range=(300, 800)), False, SCALES, 0.7, (300, 800)


def _run_case(pkg, ctx, case):
    """(device outputs, fp64 reference, schedule) of one case"""
    solver, eta, zt, n_steps, guidance, inpaint, f16 = case
    inp = _inputs()
    alphas = ZT if zt else ALPHAS
    sched = R.schedule(alphas, n_steps)
    iters = len(sched)
    g, single, scales, rescale, t_range = _guidance(pkg, guidance)
    B = N if single else 2 * N
    v = inp["v"][:iters, :B].contiguous().cuda()
    seeded_run = eta is not None
    kw = dict(solver=solver, eta=eta or 0.0, cfg_scale=7.5, guidance=g, single=single, input_f16=f16, prediction="v")
    if seeded_run:
        kw["seeds"] = SEEDS
    if inpaint:
        kw.update(reference=inp["reference"].cuda(), mask=inp["mask"].cuda())
        if not seeded_run:
            kw["step_noise"] = inp["step_noise"][:iters].contiguous().cuda()
    got = pkg.sampler_step_replay(ctx, alphas, n_steps, 0, v, inp["latent0"].cuda(), **kw)

    f64 = lambda t: t.detach().cpu().double().numpy()
    noise = lambda draw: f64(pkg.gen_noise(ctx, SEEDS, draw, N, H, W))
    active = [t_range is None or t_range[0] <= t <= t_range[1] for t, _, _ in sched]
    factors = None
    if rescale:
        factors = [f64(pkg.cfg_rescale_factors(ctx, v[i], scales, rescale)) if active[i] else None for i in range(iters)]
    blend = sigma = None
    if inpaint:
        blend = np.stack([noise(pkg.draw_blend(i)) for i in range(iters)]) if seeded_run else f64(inp["step_noise"][:iters])
    if seeded_run and eta > 0.0:
        sigma = np.stack([noise(pkg.draw_sigma(i)) for i in range(iters)])
    ref = P.replay(alphas, n_steps, 0, R.DDIM if solver == "ddim" else R.DPMPP_2M, eta or 0.0, f64(v), f64(inp["latent0"]), scales=scales,
                   active=active, factors=factors, reference=f64(inp["reference"]) if inpaint else None,
                   mask=inp["mask"].numpy() if inpaint else None, blend_noise=blend, sigma_noise=sigma)
    return got, ref, sched


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64

@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_v_kernel_against_fp64_replay(pkg, ctx, case):
    solver, eta, zt, n_steps, guidance, inpaint, f16 = case
    (latents, hist, unet_in, ts), (ref, ref_x0, M), sched = _run_case(pkg, ctx, case)
    iters = len(sched)
    for name, t in (("latents", latents), ("hist", hist), ("unet_in", unet_in), ("timesteps", ts)):
        assert torch.isfinite(t).all(), f"{name} holds a non-finite value"
    got = latents.cpu().double().numpy()
    worst = 0.0
    for i in range(iters + 1):
        err, bound = float(np.abs(got[i] - ref[i]).max()), P.U * 8 * (i + 1) * M[i]
        worst = max(worst, err / bound if bound else (0.0 if err == 0.0 else np.inf))
        assert err <= bound, f"latent {i}: max-abs error {err:.3e} over the bound {bound:.3e} (M {M[i]:.3f})"
    print(f"{_case_id(case)}: worst error / bound over {iters + 1} latents {worst:.3f}, M {M[-1]:.2f}")
    # the UNet-input copy is the last latent: NHWC, once per branch
    last = latents[-1].permute(0, 2, 3, 1).reshape(N, HW, 4)
    if f16:
        last = last.half().float()
    B = unet_in.shape[0]
    assert B == (N if guidance == "single" else 2 * N)
    assert torch.equal(unet_in.view(torch.int32), last.repeat(B // N, 1, 1).view(torch.int32))
    if solver == "dpmpp_2m":
        err, bound = float(np.abs(hist.cpu().double().numpy() - ref_x0).max()), P.U * 8 * (iters + 1) * M[-1]
        assert err <= bound, f"hist: max-abs error {err:.3e} over the bound {bound:.3e}"
    else:
        assert not hist.any()
    assert ts.cpu().tolist() == [float(t) for t, _, _ in sched] + [0.0]


# ------------------------------------------------------------------------------------------------ 2. a == 0 means x0 = -v, e = x

def test_first_iteration_at_zero_alpha(pkg, ctx):
    inp = _inputs()
    n_steps = 4
    (t, a, ap), iters = R.schedule(ZT, n_steps)[0], 4
    assert a == 0.0
    v = inp["v"][:iters].contiguous()
    latents, _, _, _ = pkg.sampler_step_replay(ctx, ZT, n_steps, 0, v.cuda(), inp["latent0"].cuda(), solver="ddim", cfg_scale=1.0, prediction="v")
    assert torch.isfinite(latents).all()
    vc, vu = (v[0, :N].double().reshape(N, H, W, 4).permute(0, 3, 1, 2).numpy(), v[0, N:].double().reshape(N, H, W, 4).permute(0, 3, 1, 2).numpy())
    vg = vu + (vc - vu) * 1.0
    x = inp["latent0"].double().numpy()
    sqrt_ap, sqrt_1map = float(np.float32(np.sqrt(ap))), float(np.float32(np.sqrt(1.0 - ap)))      # as the device holds them
    want = -sqrt_ap * vg + sqrt_1map * x
    bound = P.U * 8 * float((np.abs(sqrt_ap * vg) + np.abs(sqrt_1map * x)).max())
    err = float(np.abs(latents[1].cpu().double().numpy() - want).max())
    print(f"a == 0: latent after iteration 0 against -sqrt_ap v + sqrt_1map x: max-abs error {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ------------------------------------------------------------------------------------------------ 3. an entry alone and batched

def test_entry_alone_equals_batched(pkg, ctx):
    inp = _inputs()
    n_steps, iters = 8, 8
    kw = dict(solver="dpmpp_2m", eta=0.5, cfg_scale=7.5, prediction="v")
    v = inp["v"][:iters].contiguous()
    both = pkg.sampler_step_replay(ctx, ZT, n_steps, 0, v.cuda(), inp["latent0"].cuda(), seeds=SEEDS, **kw)
    alone = pkg.sampler_step_replay(ctx, ZT, n_steps, 0, v[:, [1, 3]].contiguous().cuda(), inp["latent0"][1:2].cuda(), seeds=SEEDS[1:], **kw)
    assert torch.isfinite(both[0]).all()
    assert torch.equal(both[0][:, 1].contiguous().view(torch.int32), alone[0][:, 0].contiguous().view(torch.int32)), "the latents of entry 1 depend on its neighbour"
    assert torch.equal(both[1][1].contiguous().view(torch.int32), alone[1][0].contiguous().view(torch.int32)), "the history of entry 1 depends on its neighbour"
    assert not torch.equal(both[0][-1, 0], both[0][-1, 1])


# ------------------------------------------------------------------------------------------------ 4. the option is a handle's

def _diffuser(pkg, ctx, ocfg, dtype, alphas=None):
    return pkg.Diffuser(ctx, to_pkg_cfg(pkg, ocfg), dtype, seed=weights_for(pkg, ocfg, dtype)[1], alphas_cumprod=alphas)


def test_prediction_is_a_handle_option(pkg, ctx):
    """the fresh handle is created after the first handle's last run, as in tests/test_gpu_solver.py's round trip"""
    ocfg, res = OC.tiny_config(), (64, 96)
    c, _ = _cond(ocfg, 2, res)
    pc = _pkg_cond(pkg, c, res)
    noise0 = pkg.gen_noise(ctx, [9, 10], pkg.DRAW_INITIAL, 2, 8, 12)
    d = _diffuser(pkg, ctx, ocfg, 1)
    assert d.get_prediction() == "epsilon"
    first = d.sample_latent(pc, 7.5, 4, noise0)
    first_seeded = d.sample_latent(pc, 7.5, 4, seeds=[9, 10], eta=0.5)
    d.set_prediction("v")
    assert d.get_prediction() == "v"
    as_v = d.sample_latent(pc, 7.5, 4, noise0)
    assert torch.isfinite(as_v).all() and not torch.equal(as_v, first)
    l = pkg.lib()
    for bad in (2, -1, 7):
        assert l.sdxl_diffuser_set_prediction(d.h, bad) == 1 and "prediction" in l.sdxl_last_error().decode()
    with pytest.raises(pkg.InvalidArgument):
        d.set_prediction(7)
    with pytest.raises(pkg.InvalidArgument):
        d.set_prediction("sample")
    v = ctypes.c_int(-1)
    assert l.sdxl_diffuser_get_prediction(d.h, ctypes.byref(v)) == 0 and v.value == pkg.PREDICTION_V
    assert l.sdxl_diffuser_get_prediction(d.h, None) == 1 and l.sdxl_diffuser_set_prediction(None, 0) == 1
    assert d.get_prediction() == "v" and torch.equal(d.sample_latent(pc, 7.5, 4, noise0), as_v), "the handle changed after refused calls"
    d.set_prediction(pkg.PREDICTION_EPSILON)
    assert d.get_prediction() == "epsilon"
    back = d.sample_latent(pc, 7.5, 4, noise0)
    assert torch.isfinite(back).all() and torch.equal(back, first), "the handle does not return to its epsilon bits"
    assert torch.equal(d.sample_latent(pc, 7.5, 4, seeds=[9, 10], eta=0.5), first_seeded)
    fresh = _diffuser(pkg, ctx, ocfg, 1)
    other = fresh.sample_latent(pc, 7.5, 4, noise0)
    assert torch.isfinite(other).all() and torch.equal(other, first), "a fresh handle gives other bits"
    assert torch.equal(fresh.sample_latent(pc, 7.5, 4, seeds=[9, 10], eta=0.5), first_seeded)


# ------------------------------------------------------------------------------------------------ 5. refusals launch nothing

def test_epsilon_on_a_zero_terminal_table_is_refused(pkg, ctx):
    ocfg, res = OC.tiny_config(), (64, 64)
    c, _ = _cond(ocfg, 1, res)
    pc = _pkg_cond(pkg, c, res)
    d = _diffuser(pkg, ctx, ocfg, 0, ZT)          # the table is taken as it is
    noise0 = pkg.gen_noise(ctx, [5], pkg.DRAW_INITIAL, 1, 8, 8)
    l = pkg.lib()
    for solver in ("ddim", "dpmpp_2m"):
        d.set_solver(solver)
        with pytest.raises(pkg.InvalidArgument, match="v-prediction"):
            d.sample_latent(pc, 7.5, 4, noise0)
        with pytest.raises(pkg.InvalidArgument, match="v-prediction"):
            d.sample_latent(pc, 7.5, 4, seeds=[5], eta=0.5)
        cc, keep = pc.to_c()
        out = torch.full((1, 4, 8, 8), 7.25, device="cuda")
        rc = l.sdxl_sample_latent(d.h, None, ctypes.byref(cc), ctypes.c_double(7.5), 4, ctypes.c_void_p(noise0.data_ptr()), ctypes.c_void_p(out.data_ptr()))
        torch.cuda.synchronize()
        assert rc == 1 and "v-prediction" in l.sdxl_last_error().decode()
        assert bool((out == 7.25).all()), "the output was written"
    # refine_latent's schedule from step_start 800 does not touch t = T - 1: the same handle runs it
    assert torch.isfinite(d.refine_latent(noise0, pc, 7.5, 800, 50, seeds=[5])).all()
    d.set_prediction("v")
    assert torch.isfinite(d.sample_latent(pc, 7.5, 4, noise0)).all()

    # the replay with prediction "epsilon": the old entry
    n, iters = 1, 4
    a = np.ascontiguousarray(ZT, dtype=np.float32)
    z = lambda *s: torch.zeros(*s, device="cuda")
    eps, latent0 = z(iters, 2 * n, 64, 4), z(n, 4, 8, 8)
    outs = [torch.full(s, 7.25, device="cuda") for s in ((iters + 1, n, 4, 8, 8), (n, 4, 8, 8), (2 * n, 64, 4), (iters + 1,))]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    args = pkg._StepReplayArgsC(a.ctypes.data_as(ctypes.c_void_p), len(a), 4, 0, pkg.SOLVER_DDIM, 0.0, 7.5, None, 0, n, 8, 8, 0, p(eps), p(latent0),
                                None, None, None, None, *[p(t) for t in outs])
    for call in (lambda: l.sdxl_sampler_step_replay(ctx.h, None, ctypes.byref(args)),
                 lambda: l.sdxl_sampler_step_replay_pred(ctx.h, None, ctypes.byref(args), pkg.PREDICTION_EPSILON)):
        assert call() == 1 and "v-prediction" in l.sdxl_last_error().decode()
        torch.cuda.synchronize()
        assert all(bool((t == 7.25).all()) for t in outs), "an output was written"
    assert l.sdxl_sampler_step_replay_pred(ctx.h, None, ctypes.byref(args), 7) == 1 and "prediction" in l.sdxl_last_error().decode()
    assert l.sdxl_sampler_step_replay_pred(ctx.h, None, ctypes.byref(args), pkg.PREDICTION_V) == 0
    with pytest.raises(pkg.InvalidArgument, match="v-prediction"):
        pkg.sampler_step_replay(ctx, ZT, 4, 0, eps, latent0, prediction="epsilon")


# ------------------------------------------------------------------------------------------------ 6. trajectories against the CPU loop

def _tables(n_steps, step_start, solver, eta):
    """(the fp64 table the trajectory runs, G)"""
    s = R.DDIM if solver == "ddim" else R.DPMPP_2M
    g_v = P.error_gain_v(P.coefficients(ZT, n_steps, step_start, s, 0.0), ZT, n_steps, step_start)
    g_eps = R.error_gain(R.coefficients(ALPHAS, n_steps, step_start, R.DDIM, 0.0), ALPHAS, n_steps, step_start)
    return P.coefficients(ZT, n_steps, step_start, s, eta), max(1.0, g_v / g_eps), g_v, g_eps


def _v_diffuser(pkg, ctx, ocfg, dtype, solver):
    d = _diffuser(pkg, ctx, ocfg, dtype, ZT)
    d.set_solver(solver)
    d.set_prediction("v")
    return d


def _report(what, out, ref, dtype, G, g_v, g_eps):
    tol = lat_tol(dtype, ref) * G
    e = max_abs(out, ref)
    print(f"{what} dtype={dtype}: latent max-abs err {e:.3e} (bar {tol:.3e}, G {G:.3f} from g_v {g_v:.2f} / g_eps {g_eps:.2f}, |latent| max {ref.abs().max():.2f})")
    assert np.isfinite(e) and e < tol


@pytest.mark.parametrize("dtype", [0, 1, 3])
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("n,n_steps,cfg_scale", [(1, 4, 7.5), (2, 8, 1.0)])
def test_v_sampling_against_cpu_loop(pkg, ctx, dtype, eta, solver, n, n_steps, cfg_scale):
    ocfg, res = OC.tiny_config(), (64, 96)
    h, w = res[0] // 8, res[1] // 8
    c, oc = _cond(ocfg, n, res)
    seeds = SEEDS[:n]
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ZT)
    table, G, g_v, g_eps = _tables(n_steps, 0, solver, eta)
    ref = P.cpu_v_loop(od, pkg, ctx, oc, cfg_scale, n_steps, seeds, eta, h, w, table)
    d = _v_diffuser(pkg, ctx, ocfg, dtype, solver)
    out = d.sample_latent(_pkg_cond(pkg, c, res), cfg_scale, n_steps, seeds=seeds, eta=eta).cpu()
    _report(f"v {solver} eta={eta} n={n} steps={n_steps}", out, ref, dtype, G, g_v, g_eps)


@pytest.mark.parametrize("dtype", [0, 3])
@pytest.mark.parametrize("solver,eta", [("ddim", 0.0), ("dpmpp_2m", 1.0)])
def test_v_refine_against_cpu_loop(pkg, ctx, dtype, solver, eta):
    """the refiner's shape: step_start 800 of 50 steps = 10 iterations on a refiner handle"""
    ocfg, res, step_start, n_steps = OC.tiny_refiner_config(), (64, 64), 800, 50
    c, oc = _cond(ocfg, 1, res, refiner=True)
    latent = seeded(1, 4, 8, 8, seed=41)
    seeds = [77]
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ZT)
    table, G, g_v, g_eps = _tables(n_steps, step_start, solver, eta)
    assert len(table) == 10
    ref = P.cpu_v_loop(od, pkg, ctx, oc, 7.5, n_steps, seeds, eta, 8, 8, table, step_start=step_start, latent0=latent)
    d = _v_diffuser(pkg, ctx, ocfg, dtype, solver)
    out = d.refine_latent(latent.cuda(), _pkg_cond(pkg, c, res, True), 7.5, step_start, n_steps, seeds=seeds, eta=eta).cpu()
    _report(f"v refine {solver} eta={eta}", out, ref, dtype, G, g_v, g_eps)


@pytest.mark.parametrize("dtype", [0, 3])
@pytest.mark.parametrize("solver,eta", [("ddim", 0.0), ("dpmpp_2m", 1.0)])
def test_v_inpainting_against_cpu_loop(pkg, ctx, dtype, solver, eta):
    ocfg, res, n_steps = OC.tiny_config(), (64, 64), 5
    c, oc = _cond(ocfg, 1, res)
    reference, mask = _inpaint_inputs()
    seeds = [4321]
    od = OP.Diffuser(ocfg, weights_for(pkg, ocfg, dtype)[0], ZT)
    table, G, g_v, g_eps = _tables(n_steps, 0, solver, eta)
    ref = P.cpu_v_loop(od, pkg, ctx, oc, 7.5, n_steps, seeds, eta, 8, 8, table, reference, mask)
    d = _v_diffuser(pkg, ctx, ocfg, dtype, solver)
    out = d.sample_latent_with_inpainting(_pkg_cond(pkg, c, res), 7.5, n_steps, reference.cuda(), mask.cuda(), seeds=seeds, eta=eta).cpu()
    _report(f"v inpainting {solver} eta={eta}", out, ref, dtype, G, g_v, g_eps)
