"""The case table of the few-step kernel tests and how one case becomes the arguments of the fp64 replay (tests/fewstep_ref.py).

Shared by tests/test_cpu_fewstep.py (an fp32 emulation of the kernel's lines stays inside the bound, on these inputs) and
tests/test_gpu_fewstep_step.py (the kernel through sdxl_sampler_step_replay_ts stays inside the same bound).  Shapes and inputs are those of
tests/sampler_step_cases.py: (2, 8, 17) is 272 threads, an entry boundary inside a wave and a ragged second block; (1, 8, 8) and (3, 8, 12)
one case each per solver.

Bound: for every recorded latent i, max|got - ref| <= 2^-24 * 8 * (i + 1) * M[i], M[i] the largest |c_x x| + |c_0 x0| + |c_z z| over the fp64
trajectory in front of latent i (the step-0 blend terms for latent 0 under inpainting).  This is the bound of tests/test_gpu_prediction.py
with the c_1 term gone: an update of a first-order row has at most eight roundings that matter (the difference and the fma of the guidance
line, the rescale product, the fma and the quotient -- or the product and the fma -- of x0, the product acc, the fma of the update, the
fma of the noise), each at most half an ulp of a value no larger than M."""
import math

import numpy as np

import fewstep_ref as F
import prediction_ref as P
import sampler_step_cases as S
from oracle import config as OC

ALPHAS = OC.alphas_cumprod()
ZT = P.rescale_zero_terminal_snr(ALPHAS)[1]
LISTS = {"L1": [999], "L4": F.schedule_lcm(4), "L8": F.schedule_lcm(8), "U4": [900, 650, 300, 20]}
CFG_SCALE = S.CFG_SCALE
SCALES = [2.0, 7.5]
RESCALE = 0.7

# (solver, gamma, prediction, zero-terminal table, guidance, inpainting, input_f16, list, shape, seeded) -- every value of every column at
# least once for each solver.  guidance: the forms of sampler_step_cases.GUIDANCE ("all": per-entry scales, rescale 0.7 and the interval
# (400, 800), which leaves 999 and 259 inactive).  Explicit noise where the table has no c_z: a one-entry LCM list, TCD at gamma = 0.
CASES = [
    ("lcm", 0.0, "epsilon", False, "scalar", False, False, "L4", (2, 8, 17), True),
    ("lcm", 0.0, "v", True, "all", True, True, "L8", (2, 8, 17), True),
    ("lcm", 0.0, "epsilon", False, "single", True, False, "L1", (2, 8, 17), False),
    ("lcm", 0.0, "v", False, "scales", False, True, "L4", (2, 8, 17), True),
    ("lcm", 0.0, "epsilon", False, "interval", True, False, "L8", (2, 8, 17), True),
    ("lcm", 0.0, "v", True, "single", False, False, "L4", (1, 8, 8), True),
    ("lcm", 0.0, "epsilon", False, "scalar", True, True, "U4", (3, 8, 12), True),
    ("tcd", 0.3, "epsilon", False, "scalar", False, False, "L4", (2, 8, 17), True),
    ("tcd", 1.0, "v", True, "all", True, True, "L8", (2, 8, 17), True),
    ("tcd", 0.0, "epsilon", False, "single", True, False, "L4", (2, 8, 17), False),
    ("tcd", 0.0, "v", False, "scales", False, True, "L1", (2, 8, 17), True),
    ("tcd", 0.3, "epsilon", False, "interval", True, False, "L8", (2, 8, 17), True),
    ("tcd", 1.0, "v", True, "single", False, False, "L4", (1, 8, 8), True),
    ("tcd", 0.3, "epsilon", False, "scalar", True, True, "U4", (3, 8, 12), True),
    ("tcd", 1.0, "epsilon", False, "all", False, False, "L4", (2, 8, 17), True),
]


def case_id(c):
    solver, gamma, pred, zt, guidance, inpaint, f16, lst, shape, seeded = c
    return "-".join([solver, f"g{gamma}", pred, "zt" if zt else "default", guidance, "inpaint" if inpaint else "free",
                     "f16in" if f16 else "f32in", lst, "%dx%dx%d" % shape, "seeded" if seeded else "explicit"])


def guidance_options(kind):
    """(keywords of make_guidance, single, per-entry scales or None, rescale, t_range or None)"""
    if kind == "single":
        return {}, True, None, 0.0, None
    k = dict(S.GUIDANCE[kind])
    return k, False, k.get("scales"), k.get("rescale", 0.0), k.get("t_range")


def rescale_factors_f64(rows, n, scales, phi):
    """f_b = phi sqrt(M2(ec_b) / M2(ecfg_b)) + 1 - phi in fp64 (the CPU stand-in for sdxl_cfg_rescale_factors: the replay and the emulation
    take the factors as given numbers)"""
    out = []
    for b in range(n):
        ec, eu = rows[b].astype(np.float64), rows[n + b].astype(np.float64)
        eg = eu + (ec - eu) * float(np.float32(scales[b]))
        m2 = lambda t: float(((t - t.mean()) ** 2).sum())
        out.append(float(np.float32(phi * math.sqrt(m2(ec) / m2(eg)) + 1.0 - phi)))
    return out


def reference_args(case, inp, blend_noise, sigma_noise, factors_of):
    """the keyword arguments fewstep_ref.replay / emulate_f32 share for one case.  inp: sampler_step_cases.make_inputs(shape); blend_noise /
    sigma_noise: callables i -> float64 [n, 4, h, w] for a seeded case (the explicit one blends with inp["step_noise"]); factors_of:
    callable (rows [2n, HW, 4] float32, scales, phi) -> n factors"""
    solver, gamma, pred, zt, guidance, inpaint, f16, lst, shape, seeded = case
    n, h, w = shape
    alphas, ts = (ZT if zt else ALPHAS), LISTS[lst]
    iters = len(ts)
    _, single, scales, rescale, t_range = guidance_options(guidance)
    if not single and scales is None:
        scales = [CFG_SCALE] * n
    rows = inp["eps"][:iters, :n] if single else inp["eps"][:iters]
    table = F.coefficients(alphas, ts, solver, gamma)
    active = [t_range is None or t_range[0] <= t <= t_range[1] for t in ts]
    factors = None
    if rescale:
        factors = [factors_of(rows[i], scales, rescale) if active[i] else None for i in range(iters)]
    kw = dict(prediction=pred, scales=scales, active=active, factors=factors)
    if inpaint:
        blend = np.stack([blend_noise(i) for i in range(iters)]) if seeded else inp["step_noise"][:iters].astype(np.float64)
        kw.update(reference=inp["reference"].astype(np.float64), mask=inp["mask"].astype(bool), blend_noise=blend)
    if seeded and np.any(table[:, 3]):
        kw["sigma_noise"] = np.stack([sigma_noise(i) for i in range(iters)])
    return alphas, ts, table, rows, kw
