"""The case matrix of tests/golden/sampler_step_bits.npz and how one case runs through sdxl_sampler_step_replay (the trajectory without the UNet).

Shared by tools/record_sampler_step_fixture.py (which wrote the fixture, once, from the three per-step kernels this project had before they became
one), tests/test_cpu_sampler_step_fixture.py (is the matrix complete, is every axis live) and tests/test_gpu_sampler_step.py (the replay).

One 256-thread block covers n * h * w pixels and b = i / HW splits entries inside a block, so the shapes are: (1, 8, 8) one partial block;
(2, 8, 17) 272 threads, two blocks with a tail and an entry boundary inside block 0; (3, 8, 12) 288 threads, two entry boundaries.

Layout of the fixture (numpy .npz, deflate):
  meta                      JSON: parent commit, hipcc version line, how it was recorded
  in/alphas                 float32 [1000]: the alphas_cumprod every case runs on
  in/<n>x<h>x<w>/...        eps [10, 2n, h*w, 4] (cond entries first, eu = ec + 0.3 noise), latent0, reference, mask (uint8), step_noise
                            [10, n, 4, h, w], seeds (uint64 [n]).  A 4-iteration case reads the first 4 of the 10; `single` the cond half of eps.
  out/<case>                float32 [n + B + (n), 4, h*w]: the final latent, the final UNet-input copy moved from [B, h*w, 4] to [B, 4, h*w] (the same
                            values in full; next to the latent in the layout of the latent the deflate window finds the copy), and under 2M the final
                            x0 history
  sha/<case>                SHA-256 of the latent stack [iterations + 1, n, 4, h, w] and of the timesteps [iterations + 1] (little-endian float32 bytes)

Toolchains: a case with explicit noise runs correctly rounded basic operations only (add, multiply, fma, divide, each written out, contraction
off), so its bits may never change, on any toolchain.  Only the seeded cases go through the device library's logf and sincosf (the Box-Muller
draw), so only they can move with a ROCm release -- and then `gen_noise` tests move with them."""
import hashlib
import itertools
import json

import numpy as np

SHAPES = [(1, 8, 8), (2, 8, 17), (3, 8, 12)]
MAIN_SHAPE = (2, 8, 17)
SCHEDULES = {"s4": (4, 0), "refiner": (50, 800)}       # (n_steps, step_start): 4 iterations, the last row has ap = 1; 10 iterations from t = 199
MAX_ITERS = 10
SOLVERS = ["ddim", "dpmpp_2m"]
NOISES = {"explicit": (False, 0.0), "seeded0": (True, 0.0), "seeded07": (True, 0.7)}      # (seeds given, eta)
# t = 999, 749, 499, 249 on s4: (400, 800) leaves 999 and 249 inactive.  scales_interval is no sixth form of the matrix: it is the no-rescale
# partner of "all", recorded for the two cases the CPU test compares it with
T_RANGE = (400, 800)
GUIDANCE = {
    "scalar": dict(),
    "single": dict(single=True),
    "scales": dict(scales=[2.0, 7.5]),
    "interval": dict(t_range=T_RANGE),
    "all": dict(rescale=0.7, scales=[2.0, 7.5], t_range=T_RANGE),
}
PARTNER = dict(scales=[2.0, 7.5], t_range=T_RANGE)
CFG_SCALE = 7.5
AXES = ("solver", "noise", "guidance", "inpaint", "shape", "schedule", "input_f16")


def case_name(c):
    return "{solver}-{noise}-{guidance}-{inp}-{n}x{h}x{w}-{schedule}-{dt}".format(
        inp="inpaint" if c["inpaint"] else "free", n=c["shape"][0], h=c["shape"][1], w=c["shape"][2], dt="f16in" if c["input_f16"] else "f32in", **c)


def _case(solver, noise, guidance, inpaint, shape=MAIN_SHAPE, schedule="s4", input_f16=False):
    return dict(solver=solver, noise=noise, guidance=guidance, inpaint=inpaint, shape=shape, schedule=schedule, input_f16=input_f16)


def matrix():
    """the full product at MAIN_SHAPE with the f32 input copy"""
    return [_case(s, z, g, i) for s, z, g, i in itertools.product(SOLVERS, NOISES, GUIDANCE, (False, True))]


def side_cases():
    """one DDIM and one 2M case (seeded eta 0.7, inpainting on) at each other shape, on the refiner schedule, and with the f16 input copy"""
    out = []
    for s in SOLVERS:
        out += [_case(s, "seeded07", "scalar", True, shape=sh) for sh in SHAPES if sh != MAIN_SHAPE]
        out += [_case(s, "seeded07", "scalar", True, schedule="refiner"), _case(s, "seeded07", "scalar", True, input_f16=True)]
    return out


def partner_cases():
    return [_case(s, "seeded07", "scales_interval", True) for s in SOLVERS]


def all_cases():
    return matrix() + side_cases() + partner_cases()


def shape_key(shape):
    return "%dx%dx%d" % tuple(shape)


def make_inputs(shape):
    """the shared inputs of one shape, as numpy arrays"""
    n, h, w = shape
    rng = np.random.default_rng(1000 * n + 10 * h + w)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    ec = f(MAX_ITERS, n, h * w, 4)
    eu = (ec + np.float32(0.3) * f(MAX_ITERS, n, h * w, 4)).astype(np.float32)       # correlated branches: the rescale factors stay away from 1
    mask = (rng.random((n, 4, h, w)) < 0.5).astype(np.uint8)
    for b in range(n):      # both values in every entry and in every 256-thread block
        flat = mask[b].reshape(4, -1)
        for lo in range(0, n * h * w, 256):
            cols = [i - b * h * w for i in range(lo, min(lo + 256, n * h * w)) if b * h * w <= i < (b + 1) * h * w]
            assert not cols or (flat[:, cols].min() == 0 and flat[:, cols].max() == 1), "degenerate mask: change the seed"
    return dict(eps=np.concatenate([ec, eu], axis=1), latent0=f(n, 4, h, w), reference=f(n, 4, h, w), mask=mask,
                step_noise=f(MAX_ITERS, n, 4, h, w), seeds=rng.integers(1, 2 ** 63, size=n, dtype=np.uint64))


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy(), dtype="<f4").tobytes()).hexdigest()


def run_case(pkg, ctx, c, inp, alphas):
    """one case through pkg.sampler_step_replay; inp: the shape's inputs as numpy arrays, alphas: float32 [1000] -> (packed float32 [n + B + (n), 4, h*w] CPU tensor,
    sha of the latent stack, sha of the timesteps)"""
    import torch
    n, h, w = c["shape"]
    n_steps, step_start = SCHEDULES[c["schedule"]]
    iters = pkg.step_count(n_steps, step_start)
    seeded, eta = NOISES[c["noise"]]
    k = dict(PARTNER if c["guidance"] == "scales_interval" else GUIDANCE[c["guidance"]])
    single = k.pop("single", False)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    eps = inp["eps"][:iters, :n] if single else inp["eps"][:iters]
    opt = dict(solver=c["solver"], eta=eta, cfg_scale=CFG_SCALE, guidance=pkg.make_guidance(**k) if k else None, single=single,
               input_f16=c["input_f16"], seeds=[int(v) for v in inp["seeds"]] if seeded else None)
    if c["inpaint"]:
        opt.update(reference=dev(inp["reference"]), mask=dev(inp["mask"]), step_noise=None if seeded else dev(inp["step_noise"][:iters]))
    latents, hist, unet_in, ts = pkg.sampler_step_replay(ctx, alphas, n_steps, step_start, dev(eps), dev(inp["latent0"]), **opt)
    assert latents.shape == (iters + 1, n, 4, h, w)
    parts = [latents[-1].reshape(n, 4, h * w), unet_in.permute(0, 2, 1)]
    if c["solver"] == "dpmpp_2m":
        parts.append(hist.reshape(n, 4, h * w))
    return torch.cat(parts).contiguous().cpu(), sha(latents), sha(ts)


def unpack(c, packed):
    """(final latent [n, 4, hw], UNet-input copy [B, 4, hw], history [n, 4, hw] or None) of a packed record"""
    n = c["shape"][0]
    B = n if c["guidance"] == "single" else 2 * n
    assert packed.shape[0] == n + B + (n if c["solver"] == "dpmpp_2m" else 0)
    return packed[:n], packed[n:n + B], packed[n + B:] if c["solver"] == "dpmpp_2m" else None


def load_meta(z):
    return json.loads(str(z["meta"]))
