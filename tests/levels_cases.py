"""The case table of the noise-level kernel tests and how one case becomes the arguments of the fp64 replay (tests/levels_ref.py).

Shared by tests/test_cpu_levels.py (an fp32 emulation of the kernel's lines stays inside the bound, on these inputs) and
tests/test_gpu_levels_step.py (the kernel through sdxl_sampler_step_replay_levels stays inside the same bound).  Shapes and inputs are those
of tests/sampler_step_cases.py: (2, 8, 17) is 272 threads, an entry boundary inside a wave and a ragged second block; (1, 8, 8) and (3, 8, 12)
one case each.

Bound: for every recorded latent i, max|got - ref| <= 2^-24 * 10 * (i + 1) * M[i], M[i] the largest |c_x x| + |c_0 x0| + |c_1 x0p| +
|c_2 x0pp| + |c_z z| over the fp64 trajectory in front of latent i (the step-0 blend terms for latent 0 under inpainting).  It is the bound
of tests/fewstep_cases.py -- eight roundings that matter in a first-order update, each at most half an ulp of a value no larger than M --
plus the two roundings the histories add: the product c_2 x0pp and the fma that adds c_1 x0p."""
import numpy as np

import fewstep_cases as FC
import levels_ref as L
import sampler_step_cases as S

ALPHAS = FC.ALPHAS
ZT = FC.ZT
CFG_SCALE = S.CFG_SCALE
ROUNDINGS = 10

_K8 = L.sigmas_karras(8, ALPHAS)
# name -> the keywords of levels_ref.levels (and of the package's entries): a sigma list or a timestep list, with its end level
SCHEDULES = {
    "K6": dict(sigmas=L.sigmas_karras(6, ALPHAS)),                        # [14.61, 6.08, 2.23, 0.693, 0.170, 0.0292]: t = 999, 837.1, 593.5, 248.8, 29.8, 0
    "K6e": dict(sigmas=_K8[:6], sigma_end=_K8[6]),                        # the first six of eight: the trajectory stops at sigma 0.0835
    "K6r": dict(sigmas=L.sigmas_karras(6, ALPHAS), round_t=True),         # the same levels, the UNet fed integer timesteps
    "E5": dict(sigmas=L.sigmas_exponential(5, ALPHAS)),
    "U4": dict(timesteps=[900, 650, 300, 20]),
    "U4e": dict(timesteps=[900, 650, 300, 20], t_end=5),
    "Z4": dict(timesteps=[999, 650, 300, 20]),                             # with the zero-terminal table: a == 0 on iteration 0 (v-prediction)
}

# (solver, eta, prediction, zero-terminal table, guidance, inpainting, input_f16, schedule, shape, seeded).  guidance: the forms of
# sampler_step_cases.GUIDANCE ("all": per-entry scales, rescale 0.7 and the interval (400, 800) on the f64 timestep).  3M on K6 and U4 at
# eta 0 and 1, explicit noise at eta 0; every column's values at least once under 3M; 2M, LCM and DDIM (eta = 1: Euler-ancestral) on sigmas.
CASES = [
    ("dpmpp_3m", 0.0, "epsilon", False, "scalar", False, False, "K6", (2, 8, 17), False),
    ("dpmpp_3m", 1.0, "epsilon", False, "scalar", False, False, "K6", (2, 8, 17), True),
    ("dpmpp_3m", 1.0, "v", True, "all", True, True, "Z4", (2, 8, 17), True),
    ("dpmpp_3m", 0.0, "v", False, "scales", False, True, "U4", (2, 8, 17), True),
    ("dpmpp_3m", 0.0, "epsilon", False, "single", True, False, "U4", (2, 8, 17), False),
    ("dpmpp_3m", 1.0, "epsilon", False, "interval", True, False, "K6", (2, 8, 17), True),
    ("dpmpp_3m", 0.0, "epsilon", False, "all", False, False, "K6e", (2, 8, 17), True),
    ("dpmpp_3m", 1.0, "epsilon", False, "scalar", False, False, "U4", (2, 8, 17), True),
    ("dpmpp_3m", 1.0, "v", False, "single", False, False, "U4e", (1, 8, 8), True),
    ("dpmpp_3m", 1.0, "epsilon", False, "scalar", True, True, "K6", (3, 8, 12), True),
    ("dpmpp_2m", 0.5, "epsilon", False, "scalar", False, False, "K6", (2, 8, 17), True),
    ("dpmpp_2m", 0.0, "v", False, "all", True, True, "K6e", (2, 8, 17), False),
    ("lcm", 0.0, "epsilon", False, "scalar", False, False, "E5", (2, 8, 17), True),
    ("ddim", 1.0, "epsilon", False, "scales", True, False, "K6r", (2, 8, 17), True),
    ("ddim", 0.0, "v", False, "single", False, True, "E5", (3, 8, 12), False),
]


def case_id(c):
    solver, eta, pred, zt, guidance, inpaint, f16, sched, shape, seeded = c
    return "-".join([solver, f"eta{eta}", pred, "zt" if zt else "default", guidance, "inpaint" if inpaint else "free",
                     "f16in" if f16 else "f32in", sched, "%dx%dx%d" % shape, "seeded" if seeded else "explicit"])


def package_schedule(pkg, sched):
    """the schedule keywords of the package's entries (solver_rows, sampler_step_replay_levels) for a SCHEDULES name"""
    k = dict(SCHEDULES[sched])
    if k.pop("round_t", False):
        k["flags"] = pkg.SIGMAS_ROUND_T
    return k


def reference_args(case, inp, blend_noise, sigma_noise, factors_of):
    """(lv, table, rows, kw): the schedule, the fp64 table and the keyword arguments levels_ref.replay / emulate_f32 share for one case.
    inp: sampler_step_cases.make_inputs(shape); blend_noise / sigma_noise: callables i -> float64 [n, 4, h, w] for a seeded case (the
    explicit one blends with inp["step_noise"]); factors_of: callable (rows [2n, HW, 4] float32, scales, phi) -> n factors"""
    solver, eta, pred, zt, guidance, inpaint, f16, sched, shape, seeded = case
    n, h, w = shape
    lv = L.levels(ZT if zt else ALPHAS, **SCHEDULES[sched])
    iters = len(lv)
    _, single, scales, rescale, t_range = FC.guidance_options(guidance)
    if not single and scales is None:
        scales = [CFG_SCALE] * n
    rows = inp["eps"][:iters, :n] if single else inp["eps"][:iters]
    table = L.coefficients(lv, solver, eta)
    active = [t_range is None or t_range[0] <= t <= t_range[1] for t, _, _ in lv]
    factors = None
    if rescale:
        factors = [factors_of(rows[i], scales, rescale) if active[i] else None for i in range(iters)]
    kw = dict(prediction=pred, scales=scales, active=active, factors=factors)
    if inpaint:
        blend = np.stack([blend_noise(i) for i in range(iters)]) if seeded else inp["step_noise"][:iters].astype(np.float64)
        kw.update(reference=inp["reference"].astype(np.float64), mask=inp["mask"].astype(bool), blend_noise=blend)
    if seeded and np.any(table[:, 4]):
        kw["sigma_noise"] = np.stack([sigma_noise(i) for i in range(iters)])
    return lv, table, rows, kw
