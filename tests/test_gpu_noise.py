"""Seeded on-device noise (sdxl_gen_noise, the *_seeded trajectories, DDIM eta) through the C ABI.

The generator is Philox4x32-10 with key = the entry's seed and counter = (hw, draw, 0, 0); tests/noise_ref.py restates it in
numpy (pinned to the published known-answer vectors by tests/test_cpu_noise.py) with the Box-Muller step in fp64.
Tiny architectures from oracle.config, bars of tests/test_gpu_models.py for whole trajectories."""
import ctypes
import math

import numpy as np
import pytest
import torch

from noise_ref import gen_noise_f64
from oracle import config as OC, pipeline as OP
from test_gpu_models import LAT_ABS_F32, _cond, _pkg_cond, lat_tol, weights_for
from util import max_abs, seeded, to_pkg_cfg

pytestmark = pytest.mark.gpu

SEEDS = [0, 1, 2, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1]
DRAWS = [0, 1, 2, 3, 200, 201]
U = 2.0 ** -24               # fp32 unit roundoff (half an ulp, relative)
ULP = 2.0 ** -23             # one fp32 ulp, relative to the value (at most)


def value_bar(z, r, theta):
    """Per-element bound on |device value - exact value|, from the documented accuracy of the device functions, not from the kernel.

    The kernel computes, in fp32 without contraction, ua and ub (exact), L = logf(ua), m = -2 L (exact), r' = sqrtf(m),
    t' = fl(2pi_f32 * ub), (s', c') = sincosf(t'), z' = fl(r' c') or fl(r' s').  The device math library is built to the OpenCL
    full-profile accuracy table: log <= 3 ulp, sqrt <= 3 ulp (HIP's default sqrtf is correctly rounded; the table value is
    used), sin / cos <= 4 ulp.
      * radius: L carries 3 ulp relative, the square root halves that and adds its own 3 ulp: |r' - r| <= 4.5 ULP r
      * angle: |t' - theta| <= theta (|2pi_f32 - 2pi| / 2pi + U) = theta (2.79e-8 + 5.96e-8) <= theta 8.75e-8; sine and cosine
        have slope <= 1, so the same bound carries to their values
      * sincosf: 4 ulp of a value in [-1, 1]: <= 4 ULP absolute
      * the final product rounds once: U relative
    |z' - z| <= r (theta 8.75e-8 + 4 ULP) + |z| (4.5 ULP + U), plus second-order terms (< 1e-11 for r <= 5.77).
    The largest bar (r = 5.77, theta = 2 pi) is 9.2e-6; a wrong counter word, key half, round count or channel order moves
    values by order 1."""
    return r * (theta * 8.75e-8 + 4 * ULP) + np.abs(z) * (4.5 * ULP + U) + 1e-11


def gpu_noise(pkg, ctx, seeds, draw, h, w):
    return pkg.gen_noise(ctx, seeds, draw, len(seeds), h, w)


@pytest.mark.parametrize("hw", [(128, 128), (12, 17)])        # latent pixels; the second is non-square with an odd width
def test_values_against_fp64_emulation(pkg, ctx, hw):
    h, w = hw
    for draw in DRAWS:
        out = gpu_noise(pkg, ctx, SEEDS, draw, h, w).cpu().numpy().astype(np.float64)
        assert out.shape == (len(SEEDS), 4, h, w)
        for b, seed in enumerate(SEEDS):
            z, r, th = gen_noise_f64(seed, draw, h, w)
            err, bar = np.abs(out[b] - z), value_bar(z, r, th)
            k = np.argmax(err / bar)
            print(f"gen_noise {h}x{w} seed={seed:#x} draw={draw}: worst |err| {err.max():.3e} (bar there {bar.flat[np.argmax(err)]:.3e}), "
                  f"worst err/bar {err.flat[k] / bar.flat[k]:.3f}, max|z| {np.abs(out[b]).max():.3f}")
            assert np.isfinite(out[b]).all()
            assert (err <= bar).all(), f"seed {seed:#x} draw {draw}: {int((err > bar).sum())} elements outside the bar"
            assert np.abs(out[b]).max() <= math.sqrt(48 * math.log(2.0)) + 1e-5


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def test_statistics(pkg, ctx):
    """30 (seed, draw) tensors of N = 4 x 128 x 128 = 65 536 GPU values.  The inputs are fixed, so the outcome is deterministic;
    the fp64 emulation alone gives worst |mean| sqrt(N) 3.04, |var - 1| sqrt(N/2) 2.38, KS D sqrt(N) 1.51, channel-pair / lag-1
    correlation sqrt(16 384) 2.84, cross-tensor correlation sqrt(N) 3.39.  Conditions: <= 5 standard errors, KS <= 1.95
    (p = 0.001 for one sample)."""
    tensors = []
    worst = dict(mean=0.0, var=0.0, ks=0.0, corr=0.0)
    for draw in DRAWS:
        out = gpu_noise(pkg, ctx, SEEDS, draw, 128, 128).cpu().double()
        for b in range(len(SEEDS)):
            g = out[b].reshape(4, -1).numpy()
            N, HW = g.size, g.shape[1]
            tensors.append(g.ravel())
            worst["mean"] = max(worst["mean"], abs(g.mean()) * math.sqrt(N))
            worst["var"] = max(worst["var"], abs(g.var() - 1.0) * math.sqrt(N / 2))
            x = np.sort(g.ravel())
            cdf = (0.5 * (1.0 + torch.special.erf(torch.from_numpy(x) / math.sqrt(2.0)))).numpy()
            i = np.arange(1, N + 1)
            D = max((i / N - cdf).max(), (cdf - (i - 1) / N).max())
            worst["ks"] = max(worst["ks"], D * math.sqrt(N))
            for a in range(4):
                for c in range(a + 1, 4):
                    worst["corr"] = max(worst["corr"], abs(_corr(g[a], g[c])) * math.sqrt(HW))
            worst["corr"] = max(worst["corr"], abs(_corr(g[0][:-1], g[0][1:])) * math.sqrt(HW))
    T = np.array(tensors)
    C = np.corrcoef(T)
    np.fill_diagonal(C, 0.0)
    cross = float(np.abs(C).max()) * math.sqrt(T.shape[1])
    print(f"statistics: |mean| sqrt(N) {worst['mean']:.2f} (<= 5), |var-1| sqrt(N/2) {worst['var']:.2f} (<= 5), KS D sqrt(N) {worst['ks']:.2f} "
          f"(<= 1.95), channel / lag-1 corr sqrt(HW) {worst['corr']:.2f} (<= 5), cross-tensor corr sqrt(N) {cross:.2f} (<= 5)")
    assert worst["mean"] <= 5 and worst["var"] <= 5 and worst["corr"] <= 5 and cross <= 5
    assert worst["ks"] <= 1.95
    for a in range(len(tensors)):
        for c in range(a + 1, len(tensors)):
            assert not np.array_equal(tensors[a], tensors[c]), f"tensors {a} and {c} are equal"


# ------------------------------------------------------------------------------------------------ seeded = explicit

def _diffuser(pkg, ctx, ocfg, dtype):
    return pkg.Diffuser(ctx, to_pkg_cfg(pkg, ocfg), dtype, seed=weights_for(pkg, ocfg, dtype)[1])


def _inpaint_inputs(n=1):
    reference = seeded(n, 4, 8, 8, seed=44)
    mask = torch.zeros(n, 4, 8, 8, dtype=torch.bool)
    mask[:, :, 0:3, :] = True      # the mask of test_sample_latent_with_inpainting
    return reference, mask


@pytest.mark.parametrize("dtype", [0, 1, 3, 5])
@pytest.mark.parametrize("n", [1, 2])
def test_seeded_sampling_equals_explicit(pkg, ctx, dtype, n):
    ocfg, res = OC.tiny_config(), (64, 96)
    c, _ = _cond(ocfg, n, res)
    seeds = [1234, 0xDEADBEEFCAFEF00D][:n]
    d = _diffuser(pkg, ctx, ocfg, dtype)
    noise0 = gpu_noise(pkg, ctx, seeds, pkg.DRAW_INITIAL, res[0] // 8, res[1] // 8)
    explicit = d.sample_latent(_pkg_cond(pkg, c, res), 7.5, 4, noise0)
    got = d.sample_latent(_pkg_cond(pkg, c, res), 7.5, 4, seeds=seeds, eta=0.0)
    assert torch.isfinite(got).all()
    assert torch.equal(got, explicit)


@pytest.mark.parametrize("dtype", [0, 1, 3, 5])
def test_seeded_refine_equals_explicit(pkg, ctx, dtype):
    ocfg, res = OC.tiny_refiner_config(), (64, 64)
    c, _ = _cond(ocfg, 1, res, refiner=True)
    latent = seeded(1, 4, 8, 8, seed=41).cuda()
    seeds = [77]
    d = _diffuser(pkg, ctx, ocfg, dtype)
    noise = gpu_noise(pkg, ctx, seeds, pkg.DRAW_INITIAL, 8, 8)
    explicit = d.refine_latent(latent, _pkg_cond(pkg, c, res, True), 7.5, 800, 50, noise)
    got = d.refine_latent(latent, _pkg_cond(pkg, c, res, True), 7.5, 800, 50, seeds=seeds)
    assert torch.isfinite(got).all()
    assert torch.equal(got, explicit)


@pytest.mark.parametrize("dtype", [0, 1, 3, 5])
def test_seeded_inpainting_equals_explicit(pkg, ctx, dtype):
    """the in-register draw of the per-step kernel against the stored step_noise tensor"""
    ocfg, res, n_steps = OC.tiny_config(), (64, 64), 5
    iters = pkg.step_count(n_steps)
    c, _ = _cond(ocfg, 1, res)
    reference, mask = _inpaint_inputs()
    seeds = [0xDEADBEEFCAFEF00D]
    d = _diffuser(pkg, ctx, ocfg, dtype)
    noise0 = gpu_noise(pkg, ctx, seeds, pkg.DRAW_INITIAL, 8, 8)
    step_noise = torch.stack([gpu_noise(pkg, ctx, seeds, pkg.draw_blend(i), 8, 8) for i in range(iters)])
    explicit = d.sample_latent_with_inpainting(_pkg_cond(pkg, c, res), 7.5, n_steps, reference.cuda(), mask.cuda(), noise0, step_noise)
    got = d.sample_latent_with_inpainting(_pkg_cond(pkg, c, res), 7.5, n_steps, reference.cuda(), mask.cuda(), seeds=seeds)
    assert torch.isfinite(got).all()
    assert torch.equal(got, explicit)


# ------------------------------------------------------------------------------------------------ batch independence

def _entry(c, i):
    return dict(ctx=c["ctx"][i:i + 1], uctx=c["uctx"], y=c["y"][i:i + 1], uy=c["uy"])


def _swapped(c):
    return dict(ctx=c["ctx"].flip(0), uctx=c["uctx"], y=c["y"].flip(0), uy=c["uy"])


@pytest.mark.parametrize("dtype", [0, 1, 3])
@pytest.mark.parametrize("inpaint", [False, True])
def test_batch_independence(pkg, ctx, dtype, inpaint):
    ocfg = OC.tiny_config()
    res, n_steps = ((64, 64), 5) if inpaint else ((64, 96), 4)
    c, _ = _cond(ocfg, 2, res)
    a, b = 1234, 0x0123456789ABCDEF
    d = _diffuser(pkg, ctx, ocfg, dtype)
    reference, mask = _inpaint_inputs(2)
    reference[1] = seeded(4, 8, 8, seed=46)

    def run(cd, seeds, sel=slice(None)):
        pc = _pkg_cond(pkg, cd, res)
        if inpaint:
            return d.sample_latent_with_inpainting(pc, 7.5, n_steps, reference[sel].cuda(), mask[sel].cuda(), seeds=seeds, eta=0.5)
        return d.sample_latent(pc, 7.5, n_steps, seeds=seeds, eta=0.5)

    both = run(c, [a, b])
    assert torch.isfinite(both).all()
    alone = run(_entry(c, 1), [b], slice(1, 2))
    assert torch.equal(alone[0], both[1]), "entry 1 depends on its batch neighbour"
    assert not torch.equal(both[0], both[1])
    # the two entries trade places (seed, conditioning, reference): the results trade places, nothing else moves
    sel = torch.tensor([1, 0])
    if inpaint:
        pc = _pkg_cond(pkg, _swapped(c), res)
        swapped = d.sample_latent_with_inpainting(pc, 7.5, n_steps, reference[sel].cuda(), mask[sel].cuda(), seeds=[b, a], eta=0.5)
    else:
        swapped = run(_swapped(c), [b, a])
    assert torch.equal(swapped[0], both[1]) and torch.equal(swapped[1], both[0])
    # swapping the seeds alone changes both entries (the seed belongs to the entry, not to the call)
    other = run(c, [b, a])
    assert not torch.equal(other[0], both[0]) and not torch.equal(other[1], both[1])
    # one seed twice with one conditioning: two equal entries
    same = dict(ctx=c["ctx"][:1].repeat(2, 1, 1), uctx=c["uctx"], y=c["y"][:1].repeat(2, 1), uy=c["uy"])
    if inpaint:
        z = torch.tensor([0, 0])
        twice = d.sample_latent_with_inpainting(_pkg_cond(pkg, same, res), 7.5, n_steps, reference[z].cuda(), mask[z].cuda(),
                                                seeds=[a, a], eta=0.5)
    else:
        twice = run(same, [a, a])
    assert torch.equal(twice[0], twice[1]) and torch.equal(twice[0], both[0])


# ------------------------------------------------------------------------------------------------ eta against a CPU loop

def _sigma(eta, a_t, a_prev):
    return eta * math.sqrt((1.0 - a_prev) / (1.0 - a_t)) * math.sqrt(1.0 - a_t / a_prev)


def cpu_eta_loop(od, pkg, ctx, oc, cfg_scale, n_steps, seeds, eta, h, w, reference=None, mask=None):
    """stablediffusion/mod.rs:390-432 (and :434-483 with a mask) in fp32 with sigma_t = eta sqrt((1-ap)/(1-a)) sqrt(1-a/ap) in place
    of the reference's 0.0, around the oracle's forward_diffuser; every noise tensor is fetched from the GPU generator.  The last
    iteration has ap = 1, so sigma = 0 and its tensor is never fetched: this is the loop "without the last draw"."""
    ts = OP.step_schedule(n_steps, 0, od.n_steps)
    step_size = od.n_steps // n_steps
    latent = gpu_noise(pkg, ctx, seeds, pkg.DRAW_INITIAL, h, w).cpu()
    for i, t in enumerate(ts):
        a_t = od.get_alpha(t)
        a_prev = od.get_alpha(t - step_size) if t >= step_size else 1.0
        sqrt_noise = (1.0 - a_t) ** 0.5
        if mask is not None:
            noised_ref = reference * (a_t ** 0.5) + gpu_noise(pkg, ctx, seeds, pkg.draw_blend(i), h, w).cpu() * sqrt_noise
            latent = torch.where(mask, latent, noised_ref)
        sigma = _sigma(eta, a_t, a_prev)
        if i == len(ts) - 1:
            assert sigma == 0.0
        eps = od.forward_diffuser(latent, t, oc, cfg_scale)
        predx0 = (latent - eps * sqrt_noise) / (a_t ** 0.5)
        latent = predx0 * (a_prev ** 0.5) + eps * ((1.0 - a_prev - sigma * sigma) ** 0.5)
        if sigma != 0.0:
            latent = latent + gpu_noise(pkg, ctx, seeds, pkg.draw_sigma(i), h, w).cpu() * sigma
    return latent


@pytest.mark.parametrize("dtype", [0, 1, 3])
@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("n,n_steps,cfg_scale", [(1, 4, 7.5), (2, 8, 1.0)])
def test_eta_against_cpu_loop(pkg, ctx, dtype, eta, n, n_steps, cfg_scale):
    """Bars of tests/test_gpu_models.py: LAT_ABS_F32 for dtypes 0 and 3, LAT_REL_F16 of max|latent| for dtype 1."""
    ocfg, res = OC.tiny_config(), (64, 96)
    h, w = res[0] // 8, res[1] // 8
    c, oc = _cond(ocfg, n, res)
    seeds = [1234, 0xDEADBEEFCAFEF00D][:n]
    W, _ = weights_for(pkg, ocfg, dtype)
    od = OP.Diffuser(ocfg, W, OC.alphas_cumprod())
    ref = cpu_eta_loop(od, pkg, ctx, oc, cfg_scale, n_steps, seeds, eta, h, w)
    d = _diffuser(pkg, ctx, ocfg, dtype)
    out = d.sample_latent(_pkg_cond(pkg, c, res), cfg_scale, n_steps, seeds=seeds, eta=eta).cpu()
    tol = lat_tol(dtype, ref)
    e = max_abs(out, ref)
    print(f"eta={eta} n={n} steps={n_steps} dtype={dtype}: latent max-abs err {e:.3e} (bar {tol:.3e}, |latent| max {ref.abs().max():.2f})")
    assert np.isfinite(e) and e < tol
    if eta == 1.0:
        plain = d.sample_latent(_pkg_cond(pkg, c, res), cfg_scale, n_steps, seeds=seeds, eta=0.0).cpu()
        moved = max_abs(out, plain)
        print(f"  eta=1 against eta=0: max-abs difference {moved:.3e}")
        assert moved > tol, "the sigma term is not live"


@pytest.mark.parametrize("dtype", [0, 3])
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_inpainting_eta_against_cpu_loop(pkg, ctx, dtype, eta):
    ocfg, res, n_steps = OC.tiny_config(), (64, 64), 5
    c, oc = _cond(ocfg, 1, res)
    reference, mask = _inpaint_inputs()
    seeds = [4321]
    W, _ = weights_for(pkg, ocfg, dtype)
    od = OP.Diffuser(ocfg, W, OC.alphas_cumprod())
    ref = cpu_eta_loop(od, pkg, ctx, oc, 7.5, n_steps, seeds, eta, 8, 8, reference, mask)
    d = _diffuser(pkg, ctx, ocfg, dtype)
    out = d.sample_latent_with_inpainting(_pkg_cond(pkg, c, res), 7.5, n_steps, reference.cuda(), mask.cuda(), seeds=seeds, eta=eta).cpu()
    e = max_abs(out, ref)
    print(f"inpainting eta={eta} dtype={dtype}: latent max-abs err {e:.3e} (bar {LAT_ABS_F32:.1e})")
    assert np.isfinite(e) and e < LAT_ABS_F32


# ------------------------------------------------------------------------------------------------ errors, determinism

def test_argument_errors(pkg, ctx):
    ocfg, res = OC.tiny_config(), (64, 64)
    c, _ = _cond(ocfg, 1, res)
    d = _diffuser(pkg, ctx, ocfg, 0)
    pc = _pkg_cond(pkg, c, res)
    cc, keep = pc.to_c()
    l = pkg.lib()
    out = torch.empty(1, 4, 8, 8, device="cuda")
    reference, mask = _inpaint_inputs()
    reference, mask = reference.cuda(), mask.to(torch.uint8).cuda()
    good = (ctypes.c_uint64 * 1)(5)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    calls = {
        "sample": lambda s, eta: l.sdxl_sample_latent_seeded(d.h, None, ctypes.byref(cc), ctypes.c_double(7.5), 4, s, ctypes.c_double(eta), p(out)),
        "inpaint": lambda s, eta: l.sdxl_sample_latent_with_inpainting_seeded(d.h, None, ctypes.byref(cc), ctypes.c_double(7.5), 4, p(reference),
                                                                              p(mask), s, ctypes.c_double(eta), p(out)),
        "refine": lambda s, eta: l.sdxl_refine_latent_seeded(d.h, None, p(reference), ctypes.byref(cc), ctypes.c_double(7.5), 800, 50, s,
                                                             ctypes.c_double(eta), p(out)),
    }
    before = d.sample_latent(pc, 7.5, 4, seeds=[5], eta=0.5)
    for name, call in calls.items():
        for s, eta in ((None, 0.0), (good, -0.1), (good, 1.5), (good, float("nan")), (good, float("inf"))):
            rc = call(s, eta)
            msg = l.sdxl_last_error().decode()
            assert rc == 1, f"{name} seeds={'NULL' if s is None else 'ok'} eta={eta}: status {rc}"        # SDXL_ERR_INVALID
            assert ("seeds" in msg) if s is None else ("eta" in msg), msg
    assert l.sdxl_gen_noise(ctx.h, None, None, ctypes.c_uint32(0), 1, 8, 8, p(out)) == 1 and "seeds" in l.sdxl_last_error().decode()
    with pytest.raises(pkg.EngineError):
        d.sample_latent(pc, 7.5, 4)                         # neither noise nor seeds
    with pytest.raises(pkg.EngineError):
        d.sample_latent(pc, 7.5, 4, seeds=[5], eta=1.5)
    assert torch.equal(d.sample_latent(pc, 7.5, 4, seeds=[5], eta=0.5), before), "the handle changed after refused calls"


@pytest.mark.parametrize("dtype", [0, 1])
def test_determinism_timing_and_trace(pkg, ctx, dtype):
    ocfg, res, n_steps = OC.tiny_config(), (64, 96), 4
    c, _ = _cond(ocfg, 2, res)
    pc = _pkg_cond(pkg, c, res)
    seeds = [9, 10]
    d1, d2 = _diffuser(pkg, ctx, ocfg, dtype), _diffuser(pkg, ctx, ocfg, dtype)
    first = d1.sample_latent(pc, 7.5, n_steps, seeds=seeds, eta=1.0)
    assert torch.equal(d1.sample_latent(pc, 7.5, n_steps, seeds=seeds, eta=1.0), first)
    assert torch.equal(d2.sample_latent(pc, 7.5, n_steps, seeds=seeds, eta=1.0), first)
    iters = pkg.step_count(n_steps)
    trace = torch.zeros(iters, 2, 4, res[0] // 8, res[1] // 8, device="cuda")
    d1.enable_step_timing(True)
    d1.set_trace(trace)
    try:
        timed = d1.sample_latent(pc, 7.5, n_steps, seeds=seeds, eta=1.0)
        ms = d1.step_times_ms()
    finally:
        d1.set_trace(None)
        d1.enable_step_timing(False)
    assert len(ms) == iters and all(m > 0 for m in ms)
    assert torch.equal(timed, first) and torch.equal(trace[iters - 1], first)
    assert all(float(trace[i].abs().max()) > 0 for i in range(iters))
