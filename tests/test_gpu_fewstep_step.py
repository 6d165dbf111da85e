"""The first-order-row instantiations of the per-step kernel (LCM and TCD) through sdxl_sampler_step_replay_ts: against the fp64 replay of
tests/fewstep_ref.py on the cases of tests/fewstep_cases.py (whose docstring states the bound and tests/test_cpu_fewstep.py checks it as a
condition), the untouched history buffer, lists against the reference's rule bit for bit for the old solvers, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fewstep_cases as C
import fewstep_ref as F
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


def _replay(pkg, ctx, case):
    """the device outputs of one case"""
    solver, gamma, pred, zt, guidance, inpaint, f16, lst, shape, seeded = case
    n, h, w = shape
    inp = _inputs(shape)
    ts = C.LISTS[lst]
    k, single, _, _, _ = C.guidance_options(guidance)
    rows = inp["eps"][:len(ts), :n] if single else inp["eps"][:len(ts)]
    opt = dict(solver=solver, eta=gamma, cfg_scale=C.CFG_SCALE, guidance=pkg.make_guidance(**k) if k else None, single=single, input_f16=f16,
               prediction=pred, timesteps=ts, seeds=[int(v) for v in inp["seeds"]] if seeded else None)
    if inpaint:
        opt.update(reference=_dev(inp["reference"]), mask=_dev(inp["mask"]), step_noise=None if seeded else _dev(inp["step_noise"][:len(ts)]))
    return pkg.sampler_step_replay(ctx, C.ZT if zt else ALPHAS, 0, 0, _dev(rows), _dev(inp["latent0"]), **opt)


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64

@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_kernel_against_fp64_replay(pkg, ctx, case):
    solver, gamma, pred, zt, guidance, inpaint, f16, lst, shape, seeded = case
    n, h, w = shape
    inp = _inputs(shape)
    seeds = [int(v) for v in inp["seeds"]]
    latents, hist, unet_in, ts_out = _replay(pkg, ctx, case)
    f64 = lambda t: t.detach().cpu().double().numpy()
    noise = lambda draw: f64(pkg.gen_noise(ctx, seeds, draw, n, h, w))
    factors_of = lambda rows, scales, phi: f64(pkg.cfg_rescale_factors(ctx, _dev(rows), scales, phi))
    alphas, ts, table, rows, kw = C.reference_args(case, inp, lambda i: noise(pkg.draw_blend(i)), lambda i: noise(pkg.draw_sigma(i)), factors_of)
    ref, M = F.replay(alphas, ts, table, rows.astype(np.float64), inp["latent0"].astype(np.float64), **kw)
    for name, t in (("latents", latents), ("unet_in", unet_in), ("timesteps", ts_out)):
        assert torch.isfinite(t).all(), f"{name} holds a non-finite value"
    got = f64(latents)
    assert got.shape == ref.shape == (len(ts) + 1, n, 4, h, w)
    worst = 0.0
    for i in range(len(ts) + 1):
        err, bound = float(np.abs(got[i] - ref[i]).max()), F.U * 8 * (i + 1) * M[i]
        worst = max(worst, err / bound if bound else (0.0 if err == 0.0 else np.inf))
        assert err <= bound, f"latent {i}: max-abs error {err:.3e} over the bound {bound:.3e} (M {M[i]:.3f})"
    print(f"{C.case_id(case)}: worst error / bound over {len(ts) + 1} latents {worst:.3f}, M {M[-1]:.2f}")
    last = latents[-1].permute(0, 2, 3, 1).reshape(n, h * w, 4)
    if f16:
        last = last.half().float()
    B = n if guidance == "single" else 2 * n
    assert unet_in.shape[0] == B and torch.equal(bits(unet_in), bits(last.repeat(B // n, 1, 1)))
    assert ts_out.cpu().tolist() == [float(t) for t in ts] + [0.0]
    assert not hist.any(), "the wrapper's zero-filled history was written"


@pytest.mark.parametrize("solver,gamma", [("lcm", 0.0), ("tcd", 0.3)])
def test_history_buffer_is_not_touched(pkg, ctx, solver, gamma):
    """hist_out pre-filled with a NaN pattern comes back bit for bit"""
    n, h, w = S.MAIN_SHAPE
    inp = _inputs(S.MAIN_SHAPE)
    ts = np.ascontiguousarray(C.LISTS["L4"], dtype=np.int32)
    a = np.ascontiguousarray(ALPHAS, dtype=np.float32)
    pattern = torch.full((n, 4, h, w), 0x7FC0BEEF, dtype=torch.int32, device="cuda")
    hist = pattern.clone()
    eps, latent0 = _dev(inp["eps"][:4]), _dev(inp["latent0"])
    outs = [torch.zeros(s, device="cuda") for s in ((5, n, 4, h, w), (2 * n, h * w, 4), (5,))]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    seeds = (ctypes.c_uint64 * n)(*[int(v) for v in inp["seeds"]])
    args = pkg._StepReplayArgsC(a.ctypes.data_as(ctypes.c_void_p), len(a), 0, 0, pkg._solver(solver), gamma, 7.5, None, 0, n, h, w, 0, p(eps), p(latent0),
                                None, None, None, ctypes.cast(seeds, ctypes.c_void_p), p(outs[0]), p(hist), p(outs[1]), p(outs[2]))
    assert pkg.lib().sdxl_sampler_step_replay_ts(ctx.h, None, ctypes.byref(args), 0, ts.ctypes.data_as(ctypes.c_void_p), 4) == 0, pkg.lib().sdxl_last_error()
    torch.cuda.synchronize()
    assert torch.equal(hist, pattern) and torch.isfinite(outs[0]).all() and outs[0][-1].abs().max() > 0


# ------------------------------------------------------------------------------------------------ 2. plumbing, bit for bit

@pytest.mark.parametrize("inpaint", [False, True])
@pytest.mark.parametrize("n_steps,step_start", [(4, 0), (50, 800)])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_explicit_reference_list_equals_no_list(pkg, ctx, solver, n_steps, step_start, inpaint):
    n, h, w = S.MAIN_SHAPE
    inp = _inputs(S.MAIN_SHAPE)
    ts = list(range(1000 - step_start - 1, -1, -(1000 // n_steps)))
    assert len(ts) == pkg.step_count(n_steps, step_start)
    opt = dict(solver=solver, eta=0.5, seeds=[int(v) for v in inp["seeds"]])
    if inpaint:
        opt.update(reference=_dev(inp["reference"]), mask=_dev(inp["mask"]))
    eps, latent0 = _dev(inp["eps"][:len(ts)]), _dev(inp["latent0"])
    old = pkg.sampler_step_replay(ctx, ALPHAS, n_steps, step_start, eps, latent0, **opt)
    new = pkg.sampler_step_replay(ctx, ALPHAS, 0, 0, eps, latent0, timesteps=ts, **opt)
    assert torch.isfinite(old[0]).all()
    for name, a, b in zip(("latents", "hist", "unet_in", "timesteps"), old, new):
        assert torch.equal(bits(a), bits(b)), f"{name} differs between the list and the rule"
    assert old[3].cpu().tolist() == [float(t) for t in ts] + [0.0]


def test_tcd_gamma0_runs_on_explicit_noise(pkg, ctx):
    inp = _inputs(S.MAIN_SHAPE)
    ts = C.LISTS["L4"]
    eps, latent0 = _dev(inp["eps"][:4]), _dev(inp["latent0"])
    tcd = pkg.sampler_step_replay(ctx, ALPHAS, 0, 0, eps, latent0, solver="tcd", timesteps=ts)
    seeded = pkg.sampler_step_replay(ctx, ALPHAS, 0, 0, eps, latent0, solver="tcd", timesteps=ts, seeds=[int(v) for v in inp["seeds"]])
    assert torch.isfinite(tcd[0]).all() and torch.equal(bits(tcd[0]), bits(seeded[0])), "gamma = 0 draws nothing: seeds change no bit"
    one = pkg.sampler_step_replay(ctx, ALPHAS, 0, 0, eps[:1], latent0, solver="lcm", timesteps=[999])
    assert torch.isfinite(one[0]).all() and not torch.equal(one[0][1], one[0][0])


def test_entry_alone_equals_batched_and_repeats(pkg, ctx):
    shape = (3, 8, 12)
    inp = _inputs(shape)
    ts = C.LISTS["L8"]
    seeds = [int(v) for v in inp["seeds"]]
    for solver, gamma in (("lcm", 0.0), ("tcd", 0.3)):
        kw = dict(solver=solver, eta=gamma, timesteps=ts)
        run = lambda sel, sd: pkg.sampler_step_replay(ctx, ALPHAS, 0, 0, _dev(inp["eps"][:8][:, sel]), _dev(inp["latent0"][[s for s in sel if s < 3]]),
                                                      seeds=sd, **kw)
        both = run([0, 1, 2, 3, 4, 5], seeds)
        again = run([0, 1, 2, 3, 4, 5], seeds)
        assert torch.isfinite(both[0]).all()
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(both, again)), "two calls give different bits"
        for b in range(3):
            alone = run([b, 3 + b], seeds[b:b + 1])
            assert torch.equal(bits(both[0][:, b]), bits(alone[0][:, 0])), f"{solver}: entry {b} depends on its neighbours"
        assert not torch.equal(both[0][-1, 0], both[0][-1, 1])


# ------------------------------------------------------------------------------------------------ 3. refusals launch nothing

def test_refusals_write_nothing(pkg, ctx):
    l = pkg.lib()
    n, h, w, iters = 1, 8, 8, 4
    a = np.ascontiguousarray(ALPHAS, dtype=np.float32)
    zt = np.ascontiguousarray(C.ZT, dtype=np.float32)
    z = lambda *s: torch.zeros(*s, device="cuda")
    eps, latent0 = z(iters, 2 * n, h * w, 4), z(n, 4, h, w)
    outs = [torch.full(s, 7.25, device="cuda") for s in ((iters + 1, n, 4, h, w), (n, 4, h, w), (2 * n, h * w, 4), (iters + 1,))]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    seeds = (ctypes.c_uint64 * n)(5)

    def call(ts=(999, 759, 499, 259), alphas=a, solver=pkg.SOLVER_LCM, eta=0.0, seeded=True, prediction=0):
        t = np.ascontiguousarray(ts, dtype=np.int32)
        args = pkg._StepReplayArgsC(alphas.ctypes.data_as(ctypes.c_void_p), 1000, 0, 0, solver, eta, 7.5, None, 0, n, h, w, 0, p(eps), p(latent0),
                                    None, None, None, ctypes.cast(seeds, ctypes.c_void_p) if seeded else None, *[p(o) for o in outs])
        rc = l.sdxl_sampler_step_replay_ts(ctx.h, None, ctypes.byref(args), prediction, t.ctypes.data_as(ctypes.c_void_p), len(ts))
        torch.cuda.synchronize()
        return rc, l.sdxl_last_error().decode()

    refused = [(dict(seeded=False), "seeded"), (dict(solver=pkg.SOLVER_TCD, eta=0.3, seeded=False), "seeds"),
               (dict(ts=(999, 499, 499, 259)), "timesteps"), (dict(ts=(259, 499, 759, 999)), "timesteps"), (dict(ts=(1000, 759, 499, 259)), "timesteps"),
               (dict(eta=0.5), "eta"), (dict(alphas=zt), "v-prediction"), (dict(alphas=zt, solver=pkg.SOLVER_TCD), "v-prediction"),
               (dict(solver=2), "solver"), (dict(solver=7), "solver")]
    for kw, word in refused:
        rc, msg = call(**kw)
        assert rc == 1 and word in msg, (kw, rc, msg)
        assert all(bool((o == 7.25).all()) for o in outs), f"{kw}: an output was written"
    rc, msg = call(alphas=zt, prediction=1)
    assert rc == 0, msg
    assert all(bool(torch.isfinite(o).all()) for o in outs) and not bool((outs[0] == 7.25).any())
    with pytest.raises(pkg.InvalidArgument, match="seeded"):
        pkg.sampler_step_replay(ctx, ALPHAS, 0, 0, eps, latent0, solver="lcm", timesteps=[999, 759, 499, 259])


def test_handle_refuses_a_call_that_disagrees_with_its_list(pkg, ctx):
    """n_steps not equal to the list's length, eta under LCM, explicit noise with c_z != 0: SDXL_ERR_INVALID and an untouched output"""
    from test_gpu_models import _cond, _pkg_cond, weights_for
    from util import to_pkg_cfg
    ocfg, res = OC.tiny_config(), (64, 64)
    c, _ = _cond(ocfg, 1, res)
    pc = _pkg_cond(pkg, c, res)
    d = pkg.Diffuser(ctx, to_pkg_cfg(pkg, ocfg), 0, seed=weights_for(pkg, ocfg, 0)[1])
    d.set_solver("lcm")
    d.set_timesteps([999, 759, 499, 259])
    l = pkg.lib()
    cc, keep = pc.to_c()
    out = torch.full((1, 4, 8, 8), 7.25, device="cuda")
    seeds = (ctypes.c_uint64 * 1)(5)
    noise0 = pkg.gen_noise(ctx, [5], pkg.DRAW_INITIAL, 1, 8, 8)
    seeded_call = lambda n_steps, eta: l.sdxl_sample_latent_seeded(d.h, None, ctypes.byref(cc), ctypes.c_double(1.0), n_steps, seeds, ctypes.c_double(eta),
                                                                   ctypes.c_void_p(out.data_ptr()))
    for call, word in ((lambda: seeded_call(3, 0.0), "timesteps"), (lambda: seeded_call(5, 0.0), "timesteps"), (lambda: seeded_call(4, 0.5), "eta"),
                       (lambda: l.sdxl_sample_latent(d.h, None, ctypes.byref(cc), ctypes.c_double(1.0), 4, ctypes.c_void_p(noise0.data_ptr()),
                                                     ctypes.c_void_p(out.data_ptr())), "seeded")):
        rc = call()
        torch.cuda.synchronize()
        assert rc == 1 and word in l.sdxl_last_error().decode(), l.sdxl_last_error().decode()
        assert bool((out == 7.25).all()), "the output was written"
    assert seeded_call(4, 0.0) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not bool((out == 7.25).any())
