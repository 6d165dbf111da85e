"""The per-step kernel on noise-level schedules through sdxl_sampler_step_replay_levels: the DPM++ 3M SDE instantiations, and 2M, LCM and
DDIM on sigma lists, against the fp64 replay of tests/levels_ref.py on the cases of tests/levels_cases.py (whose docstring states the bound
and tests/test_cpu_levels.py checks it as a condition); the two history buffers; the fractional timesteps; an integer list against
sdxl_sampler_step_replay_ts bit for bit; and the refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fewstep_cases as FC
import levels_cases as C
import levels_ref as L
import sampler_step_cases as S
from oracle import config as OC

pytestmark = pytest.mark.gpu

ALPHAS = OC.alphas_cumprod()
bits = lambda t: t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    return S.make_inputs(shape)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _replay(pkg, ctx, case, **extra):
    """the device outputs of one case"""
    solver, eta, pred, zt, guidance, inpaint, f16, sched, shape, seeded = case
    n, h, w = shape
    inp = _inputs(shape)
    k = C.package_schedule(pkg, sched)
    iters = len(k["sigmas"] if "sigmas" in k else k["timesteps"])
    g, single, _, _, _ = FC.guidance_options(guidance)
    rows = inp["eps"][:iters, :n] if single else inp["eps"][:iters]
    opt = dict(solver=solver, eta=eta, cfg_scale=C.CFG_SCALE, guidance=pkg.make_guidance(**g) if g else None, single=single, input_f16=f16,
               prediction=pred, seeds=[int(v) for v in inp["seeds"]] if seeded else None, **k, **extra)
    if inpaint:
        opt.update(reference=_dev(inp["reference"]), mask=_dev(inp["mask"]), step_noise=None if seeded else _dev(inp["step_noise"][:iters]))
    return pkg.sampler_step_replay_levels(ctx, C.ZT if zt else ALPHAS, _dev(rows), _dev(inp["latent0"]), **opt)


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64

@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_kernel_against_fp64_replay(pkg, ctx, case):
    solver, eta, pred, zt, guidance, inpaint, f16, sched, shape, seeded = case
    n, h, w = shape
    inp = _inputs(shape)
    seeds = [int(v) for v in inp["seeds"]]
    latents, hist, hist2, unet_in, ts_out = _replay(pkg, ctx, case, hist_fill=float("nan"))
    f64 = lambda t: t.detach().cpu().double().numpy()
    noise = lambda draw: f64(pkg.gen_noise(ctx, seeds, draw, n, h, w))
    factors_of = lambda rows, scales, phi: f64(pkg.cfg_rescale_factors(ctx, _dev(rows), scales, phi))
    lv, table, rows, kw = C.reference_args(case, inp, lambda i: noise(pkg.draw_blend(i)), lambda i: noise(pkg.draw_sigma(i)), factors_of)
    ref, M, ref_hist, ref_hist2 = L.replay(lv, solver, table, rows.astype(np.float64), inp["latent0"].astype(np.float64), **kw)
    for name, t in (("latents", latents), ("unet_in", unet_in), ("timesteps", ts_out)):
        assert torch.isfinite(t).all(), f"{name} holds a non-finite value"
    got = f64(latents)
    assert got.shape == ref.shape == (len(lv) + 1, n, 4, h, w)
    worst = 0.0
    for i in range(len(lv) + 1):
        err, bound = float(np.abs(got[i] - ref[i]).max()), L.U * C.ROUNDINGS * (i + 1) * M[i]
        worst = max(worst, err / bound if bound else (0.0 if err == 0.0 else np.inf))
        assert err <= bound, f"latent {i}: max-abs error {err:.3e} over the bound {bound:.3e} (M {M[i]:.3f})"
    print(f"{C.case_id(case)}: worst error / bound over {len(lv) + 1} latents {worst:.3f}, M {M[-1]:.2f}")
    last = latents[-1].permute(0, 2, 3, 1).reshape(n, h * w, 4)
    if f16:
        last = last.half().float()
    B = n if guidance == "single" else 2 * n
    assert unet_in.shape[0] == B and torch.equal(bits(unet_in), bits(last.repeat(B // n, 1, 1)))
    # the timestep the UNet is fed: (float)t of every entry, fractional on a sigma list, bit for bit; 0 behind the last
    want_t = torch.tensor([np.float32(t) for t, _, _ in lv] + [np.float32(0.0)], dtype=torch.float32)
    assert torch.equal(bits(ts_out.cpu()), bits(want_t))
    if "sigmas" in C.SCHEDULES[sched] and not C.SCHEDULES[sched].get("round_t"):
        assert any(float(t) != round(float(t)) for t in want_t), "a sigma list feeds fractional timesteps"
    # the histories by the kernel's rule: hist the x0 of the last update, hist2 the x0 in front of the last update that read a history
    # (c_1 != 0) -- each recomputed in fp64 from the latent the device recorded in front of that update (levels_ref.x0_with_bound)
    untouched = lambda t: bool(torch.isnan(t).all())
    gkw = {k: kw[k] for k in ("prediction", "scales", "active", "factors")}
    if solver in ("dpmpp_2m", "dpmpp_3m"):
        x0, tol = L.x0_with_bound(lv, len(lv) - 1, got[len(lv) - 1], rows, **gkw)
        assert np.abs(f64(hist) - x0).max() <= tol
        # and that x0 is the reference trajectory's: the latent in front of the update is within its bound B, x0 divides it by sqrt_a (v: times it)
        B, sa = L.U * C.ROUNDINGS * len(lv) * M[len(lv) - 1], float(np.float32(np.sqrt(lv[-1][1])))
        assert np.abs(x0 - ref_hist).max() <= B / sa * (1.0 + 1e-9)
        shifts = [i for i in range(len(lv)) if np.float32(table[i][2]) != 0]
        if solver == "dpmpp_3m" and shifts:
            x0, tol = L.x0_with_bound(lv, shifts[-1] - 1, got[shifts[-1] - 1], rows, **gkw)
            assert np.abs(f64(hist2) - x0).max() <= tol and not np.array_equal(f64(hist), f64(hist2))
        else:
            assert untouched(hist2), "the second history was written by a solver that keeps none"
    else:
        assert untouched(hist) and untouched(hist2), "a history was written by a solver that keeps none"


def test_histories_hold_the_last_two_x0(pkg, ctx):
    """3M on a list with an end level, explicit noise, one branch: x0 of the last two iterations recomputed from the recorded latents"""
    n, h, w = S.MAIN_SHAPE
    inp = _inputs(S.MAIN_SHAPE)
    k = C.package_schedule(pkg, "K6e")
    lv = L.levels(ALPHAS, **C.SCHEDULES["K6e"])
    rows = inp["eps"][:6, :n]
    latents, hist, hist2, _, _ = pkg.sampler_step_replay_levels(ctx, ALPHAS, _dev(rows), _dev(inp["latent0"]), solver="dpmpp_3m", single=True, **k)
    f = np.float32
    for buf, i in ((hist, 5), (hist2, 4)):
        x = latents[i].cpu().numpy()
        e = rows[i].reshape(n, h, w, 4).transpose(0, 3, 1, 2)
        sa, s1 = f(np.sqrt(lv[i][1])), f(np.sqrt(1.0 - lv[i][1]))
        x0 = L._fma32(-e, s1, x) / sa          # the kernel's x0 line on the recorded fp32 latent: bit for bit
        assert np.array_equal(buf.cpu().numpy().view(np.int32), x0.view(np.int32)), f"history of iteration {i}"


# ------------------------------------------------------------------------------------------------ 2. plumbing, bit for bit

@pytest.mark.parametrize("inpaint", [False, True])
@pytest.mark.parametrize("solver,eta", [("ddim", 0.5), ("dpmpp_2m", 0.5), ("lcm", 0.0), ("tcd", 0.3)])
def test_integer_list_gives_the_bits_of_the_ts_entry(pkg, ctx, solver, eta, inpaint):
    n, h, w = S.MAIN_SHAPE
    inp = _inputs(S.MAIN_SHAPE)
    ts = [900, 650, 300, 20]
    opt = dict(solver=solver, eta=eta, seeds=[int(v) for v in inp["seeds"]])
    if inpaint:
        opt.update(reference=_dev(inp["reference"]), mask=_dev(inp["mask"]))
    eps, latent0 = _dev(inp["eps"][:4]), _dev(inp["latent0"])
    old = pkg.sampler_step_replay(ctx, ALPHAS, 0, 0, eps, latent0, timesteps=ts, **opt)
    new = pkg.sampler_step_replay_levels(ctx, ALPHAS, eps, latent0, timesteps=ts, **opt)
    assert torch.isfinite(old[0]).all()
    for name, a, b in zip(("latents", "hist", "unet_in", "timesteps"), old, (new[0], new[1], new[3], new[4])):
        assert torch.equal(bits(a), bits(b)), f"{name} differs between the two entries"
    assert not new[2].any(), "the second history was written"


def test_end_level_changes_only_the_last_update(pkg, ctx):
    inp = _inputs(S.MAIN_SHAPE)
    eps, latent0 = _dev(inp["eps"][:4]), _dev(inp["latent0"])
    for solver in ("ddim", "dpmpp_2m", "dpmpp_3m"):
        full = pkg.sampler_step_replay_levels(ctx, ALPHAS, eps, latent0, solver=solver, timesteps=[900, 650, 300, 20])
        cut = pkg.sampler_step_replay_levels(ctx, ALPHAS, eps, latent0, solver=solver, timesteps=[900, 650, 300, 20], t_end=5)
        assert torch.equal(bits(full[0][:4]), bits(cut[0][:4])) and not torch.equal(full[0][4], cut[0][4])
        # the first four entries of a six-entry list with the fifth as the end level: the first four updates of the six-entry run
        six = pkg.sampler_step_replay_levels(ctx, ALPHAS, _dev(inp["eps"][:6]), latent0, solver=solver, timesteps=[900, 650, 300, 20, 10, 5])
        four = pkg.sampler_step_replay_levels(ctx, ALPHAS, eps, latent0, solver=solver, timesteps=[900, 650, 300, 20], t_end=10)
        assert torch.equal(bits(six[0][:5]), bits(four[0]))


def test_entry_alone_equals_batched_and_repeats(pkg, ctx):
    shape = (3, 8, 12)
    inp = _inputs(shape)
    seeds = [int(v) for v in inp["seeds"]]
    k = C.package_schedule(pkg, "K6")
    run = lambda sel, sd: pkg.sampler_step_replay_levels(ctx, ALPHAS, _dev(inp["eps"][:6][:, sel]), _dev(inp["latent0"][[s for s in sel if s < 3]]),
                                                         solver="dpmpp_3m", eta=1.0, seeds=sd, **k)
    both = run([0, 1, 2, 3, 4, 5], seeds)
    again = run([0, 1, 2, 3, 4, 5], seeds)
    assert torch.isfinite(both[0]).all()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(both, again)), "two calls give different bits"
    for b in range(3):
        alone = run([b, 3 + b], seeds[b:b + 1])
        assert torch.equal(bits(both[0][:, b]), bits(alone[0][:, 0])), f"entry {b} depends on its neighbours"
        assert torch.equal(bits(both[2][b]), bits(alone[2][0]))
    assert not torch.equal(both[0][-1, 0], both[0][-1, 1])


# ------------------------------------------------------------------------------------------------ 3. refusals launch nothing

def test_refusals_write_nothing(pkg, ctx):
    l = pkg.lib()
    n, h, w, iters = 1, 8, 8, 6
    z = lambda *s: torch.zeros(*s, device="cuda")
    eps, latent0 = z(iters, 2 * n, h * w, 4), z(n, 4, h, w)
    outs = [torch.full(s, 7.25, device="cuda") for s in ((iters + 1, n, 4, h, w), (n, 4, h, w), (2 * n, h * w, 4), (iters + 1,), (n, 4, h, w))]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    seeds = (ctypes.c_uint64 * n)(5)
    K6 = L.sigmas_karras(6, ALPHAS)
    a32 = np.ascontiguousarray(ALPHAS, dtype=np.float32)

    def call(solver=pkg.SOLVER_DPMPP_3M, eta=0.0, seeded=True, prediction=0, alphas=ALPHAS, old_entry=False, **k):
        if not k:
            k = dict(sigmas=K6)
        desc, keep, cnt = pkg._schedule_desc(alphas, **k)
        args = pkg._StepReplayArgsC(a32.ctypes.data_as(ctypes.c_void_p), 1000, 0, 0, solver, eta, 7.5, None, 0, n, h, w, 0, p(eps), p(latent0),
                                    None, None, None, ctypes.cast(seeds, ctypes.c_void_p) if seeded else None, *[p(o) for o in outs[:4]])
        if old_entry:
            ts = np.ascontiguousarray([999, 800, 600, 400, 200, 0], dtype=np.int32)
            rc = l.sdxl_sampler_step_replay_ts(ctx.h, None, ctypes.byref(args), prediction, ts.ctypes.data_as(ctypes.c_void_p), 6)
        else:
            rc = l.sdxl_sampler_step_replay_levels(ctx.h, None, ctypes.byref(args), prediction, ctypes.byref(desc), p(outs[4]))
        torch.cuda.synchronize()
        return rc, l.sdxl_last_error().decode()

    refused = [(dict(solver=pkg.SOLVER_TCD, eta=0.3), "sigmas"), (dict(solver=pkg.SOLVER_LCM, seeded=False), "seeded"), (dict(eta=0.5, seeded=False), "seeds"),
               (dict(sigmas=[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), "sigmas"), (dict(sigmas=K6, sigma_end=1.0), "sigmas"), (dict(sigmas=K6, flags=4), "sigmas"),
               (dict(timesteps=[999, 800, 600, 400, 200, 100], t_end=100), "timesteps"), (dict(timesteps=[999, 800, 600, 400, 200, 100], sigmas=K6), "exactly one"),
               (dict(solver=2), "solver"), (dict(solver=7), "solver"), (dict(eta=1.5), "eta"), (dict(prediction=3), "prediction"),
               (dict(timesteps=[999, 800, 600, 400, 200, 100], alphas=FC.ZT), "v-prediction"), (dict(old_entry=True), "sdxl_sampler_step_replay_levels")]
    for kw, word in refused:
        rc, msg = call(**kw)
        assert rc == 1 and word in msg, (kw, rc, msg)
        assert all(bool((o == 7.25).all()) for o in outs), f"{kw}: an output was written"
    rc, msg = call()
    assert rc == 0, msg
    assert all(bool(torch.isfinite(o).all()) for o in outs) and not bool((outs[0] == 7.25).any()) and not bool((outs[4] == 7.25).any())
