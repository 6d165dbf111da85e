"""fp64 numpy restatement of few-step sampling (include/sdxl_mi355.h, the few-step section), written from the formulas there and not
from the C++: the four timestep spacings, (t, a, ap) from a list, the LCM and TCD rows and the DDIM and DPM-Solver++(2M) rows on a list,
an fp64 replay and an fp32 emulation of the per-step arithmetic of the first-order rows, and a CPU trajectory loop on a list.

A list t_0 > t_1 > ... is the only source of an iteration's numbers: a = alphas[t_i], ap = alphas[t_{i+1}], ap = 1 behind the last entry.
One iteration is x' = c_x x + c_0 x0 + c_1 x0p + c_z z with x0 = (x - sigma e) / alpha (epsilon) or alpha x - sigma v (v-prediction);
alpha = sqrt(a), sigma = sqrt(1 - a), primes for ap.

    LCM   s = 10 t, c_skip = 0.25 / (s^2 + 0.25), c_out = s / sqrt(s^2 + 0.25):  (alpha' c_skip, alpha' c_out, 0, sigma')
    TCD   t' the next entry, s = floor((1 - gamma) t'), a_s = alphas[s], r = sqrt(ap / a_s):
          (r sigma_s / sigma, r (alpha_s - sigma_s alpha / sigma), 0, sqrt(1 - ap / a_s));  behind the last entry (0, 1, 0, 0)"""
import math

import numpy as np
import torch

import prediction_ref as P
import solver_ref as R

DDIM, DPMPP_2M, LCM, TCD = 0, 1, 3, 4
SOLVERS = {"ddim": DDIM, "dpmpp_2m": DPMPP_2M, "lcm": LCM, "tcd": TCD}
U = P.U


# ------------------------------------------------------------------------------------------------ spacings

def schedule_reference(n_steps, n_train=1000):
    return list(range(n_train - 1, -1, -(n_train // n_steps)))


def schedule_trailing(n_steps, n_train=1000):
    q = float(n_train) / float(n_steps)
    return [int(np.rint(float(n_train) - float(i) * q)) - 1 for i in range(n_steps)]       # rint: ties to even


def schedule_leading(n_steps, n_train=1000, offset=1):
    return [(n_steps - 1 - i) * (n_train // n_steps) + offset for i in range(n_steps)]


def schedule_lcm(n_steps, n_train=1000, origin_steps=50):
    k = n_train // origin_steps
    return [(origin_steps - (i * origin_steps) // n_steps) * k - 1 for i in range(n_steps)]


def timestep_schedule(kind, n_steps, n_train=1000, offset=1, origin_steps=50):
    return {"reference": lambda: schedule_reference(n_steps, n_train), "trailing": lambda: schedule_trailing(n_steps, n_train),
            "leading": lambda: schedule_leading(n_steps, n_train, offset), "lcm": lambda: schedule_lcm(n_steps, n_train, origin_steps)}[kind]()


def schedule(alphas, ts):
    """[(t, a, ap)] of a list"""
    alphas = np.asarray(alphas, dtype=np.float32).astype(np.float64)
    ts = [int(t) for t in ts]
    assert all(0 <= t < len(alphas) for t in ts) and all(b < a for a, b in zip(ts, ts[1:]))
    return [(t, float(alphas[t]), float(alphas[ts[i + 1]]) if i + 1 < len(ts) else 1.0) for i, t in enumerate(ts)]


# ------------------------------------------------------------------------------------------------ tables

def lcm_rows(alphas, ts):
    rows = []
    for t, a, ap in schedule(alphas, ts):
        s = 10.0 * t
        c_skip, c_out = 0.25 / (s * s + 0.25), s / math.sqrt(s * s + 0.25)
        rows.append((math.sqrt(ap) * c_skip, math.sqrt(ap) * c_out, 0.0, math.sqrt(1.0 - ap)))
    return np.array(rows, dtype=np.float64)


def tcd_rows(alphas, ts, gamma):
    al = np.asarray(alphas, dtype=np.float32).astype(np.float64)
    rows = []
    for i, (t, a, ap) in enumerate(schedule(alphas, ts)):
        if i + 1 == len(ts):
            rows.append((0.0, 1.0, 0.0, 0.0))
            continue
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        a_s = float(al[int(math.floor((1.0 - gamma) * ts[i + 1]))])
        alpha_s, sigma_s, r = math.sqrt(a_s), math.sqrt(1.0 - a_s), math.sqrt(ap / a_s)
        rows.append((r * sigma_s / sigma, r * (alpha_s - sigma_s * alpha / sigma), 0.0, math.sqrt(max(1.0 - ap / a_s, 0.0))))
    return np.array(rows, dtype=np.float64)


def ddim_rows(alphas, ts, eta=0.0):
    rows = []
    for t, a, ap in schedule(alphas, ts):
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        sqrt_ap, sqrt_1map, sigma_t = R.ddim_terms(a, ap, eta)
        rows.append((sqrt_1map / sigma, sqrt_ap - sqrt_1map * alpha / sigma, 0.0, sigma_t))
    return np.array(rows, dtype=np.float64)


def dpmpp2m_rows(alphas, ts, eta=0.0):
    """the rows of solver_ref / prediction_ref (a == 0 admitted) with (a, ap) from the list"""
    rows, h_prev = [], None
    for t, a, ap in schedule(alphas, ts):
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        if ap == 1.0:
            rows.append((0.0, 1.0, 0.0, 0.0))
            h_prev = None
            continue
        alpha_p, sigma_p = math.sqrt(ap), math.sqrt(1.0 - ap)
        if a == 0.0:
            rows.append((sigma_p, alpha_p, 0.0, 0.0) if eta == 0.0 else (0.0, alpha_p, 0.0, sigma_p))
            h_prev = None
            continue
        h = math.log(alpha_p / sigma_p) - math.log(alpha / sigma)
        A = -math.expm1(-(1.0 + eta) * h)
        c_x, c_z = (sigma_p / sigma) * math.exp(-eta * h), sigma_p * math.sqrt(-math.expm1(-2.0 * eta * h))
        if h_prev is None:
            c_0, c_1 = alpha_p * A, 0.0
        else:
            r = h_prev / h
            c_0, c_1 = alpha_p * A * (1.0 + 1.0 / (2.0 * r)), -alpha_p * A / (2.0 * r)
        rows.append((c_x, c_0, c_1, c_z))
        h_prev = h
    return np.array(rows, dtype=np.float64)


def coefficients(alphas, ts, solver, eta=0.0):
    """[len(ts), 4] float64 rows (c_x, c_0, c_1, c_z); eta is gamma under TCD and must be 0 under LCM"""
    solver = SOLVERS.get(solver, solver)
    if solver == LCM:
        assert eta == 0.0
        return lcm_rows(alphas, ts)
    if solver == TCD:
        return tcd_rows(alphas, ts, eta)
    return ddim_rows(alphas, ts, eta) if solver == DDIM else dpmpp2m_rows(alphas, ts, eta)


def error_gain(table, alphas, ts, prediction="epsilon"):
    """the first-order gain of a UNet-output error onto the latent: sum_i (|c_0,i| k_i + |c_1,i| k_{i-1}), k = sigma / alpha under epsilon
    (solver_ref.error_gain) and sigma under v (prediction_ref.error_gain_v)"""
    k = [math.sqrt(1.0 - a) / (math.sqrt(a) if prediction == "epsilon" else 1.0) for _, a, _ in schedule(alphas, ts)]
    return sum(abs(table[i][1]) * k[i] + (abs(table[i][2]) * k[i - 1] if i else 0.0) for i in range(len(k)))


# ------------------------------------------------------------------------------------------------ the per-step arithmetic of a first-order row

def _f32(x):
    return float(np.float32(x))


def replay(alphas, ts, table, rows_in, latent0, prediction="epsilon", scales=None, active=None, factors=None, reference=None, mask=None,
           blend_noise=None, sigma_noise=None):
    """prediction_ref.replay for a first-order table on a list and both prediction types: fp64 arithmetic on what the device holds (the
    table row, sqrt_a and sqrt_1ma rounded to fp32).  rows_in [iters, B, HW, 4] the network's rows (e or v), B = n or 2n (cond entries
    first); the other arguments as in prediction_ref.replay.  Returns (latents [iters + 1, n, 4, h, w], M [iters + 1]): M[i] the largest
    |c_x x| + |c_0 x0| + |c_z z| over the updates in front of recorded latent i; M[0] the size of the step-0 blend terms (0 without)."""
    s = schedule(alphas, ts)
    iters = len(s)
    assert len(table) == iters and not np.any(np.asarray(table)[:, 2])
    n, _, h, w = latent0.shape
    x = latent0.astype(np.float64).copy()
    rows = lambda i, b: rows_in[i, b].reshape(h, w, 4).transpose(2, 0, 1)

    def blend(x, i):
        sa, s1 = _f32(math.sqrt(s[i][1])), _f32(math.sqrt(1.0 - s[i][1]))
        return np.where(mask, x, reference * sa + blend_noise[i] * s1), float((np.abs(reference * sa) + np.abs(blend_noise[i] * s1)).max())

    M, m = [0.0], 0.0
    if mask is not None:
        x, M[0] = blend(x, 0)
    latents = [x.copy()]
    for i, (t, a, ap) in enumerate(s):
        sa, s1 = _f32(math.sqrt(a)), _f32(math.sqrt(1.0 - a))
        on = scales is not None and (active is None or bool(active[i]))
        e = np.empty_like(x)
        for b in range(n):
            e[b] = rows(i, b)
            if on:
                eu = rows(i, n + b)
                e[b] = eu + (e[b] - eu) * _f32(scales[b])
                if factors is not None and factors[i] is not None:
                    e[b] = e[b] * float(factors[i][b])
        x0 = x * sa - e * s1 if prediction == "v" else (x - e * s1) / sa
        c_x, c_0, _, c_z = (_f32(c) for c in table[i])
        terms = np.abs(x * c_x) + np.abs(x0 * c_0)
        x = x * c_x + x0 * c_0
        if sigma_noise is not None and c_z != 0.0:
            terms = terms + np.abs(sigma_noise[i] * c_z)
            x = x + sigma_noise[i] * c_z
        m = max(m, float(terms.max()))
        if mask is not None and i + 1 < iters:
            x, _ = blend(x, i + 1)
        latents.append(x.copy())
        M.append(m)
    return np.stack(latents), np.array(M)


def _fma32(a, b, c):
    """fp32 fma of fp32 arrays: the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double
    rounding differs from the fused one in about one case in 2^29: nothing a bound with a margin notices)"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def emulate_f32(alphas, ts, table, rows_in, latent0, prediction="epsilon", scales=None, active=None, factors=None, reference=None, mask=None,
                blend_noise=None, sigma_noise=None):
    """the lines of the per-step kernel for a first-order row in fp32 numpy, rounding by rounding as the header states them:
    e = fma(ec - eu, s_b, eu) (* f_b);  x0 = fma(-e, sqrt_1ma, x) / sqrt_a  or  fma(x, sqrt_a, -(v sqrt_1ma));  acc = x0 c_0;
    x = fma(x, c_x, acc);  x = fma(z, c_z, x);  the blend rounds both products.  Inputs float32; returns latents float32 [iters + 1, ...]"""
    f = np.float32
    s = schedule(alphas, ts)
    iters = len(s)
    n, _, h, w = latent0.shape
    x = latent0.astype(f).copy()
    rows = lambda i, b: rows_in[i, b].reshape(h, w, 4).transpose(2, 0, 1).astype(f)

    def blend(x, i):
        sa, s1 = f(math.sqrt(s[i][1])), f(math.sqrt(1.0 - s[i][1]))
        return np.where(mask, x, (reference.astype(f) * sa + blend_noise[i].astype(f) * s1).astype(f))

    if mask is not None:
        x = blend(x, 0)
    latents = [x.copy()]
    for i, (t, a, ap) in enumerate(s):
        sa, s1 = f(math.sqrt(a)), f(math.sqrt(1.0 - a))
        on = scales is not None and (active is None or bool(active[i]))
        e = np.empty_like(x)
        for b in range(n):
            e[b] = rows(i, b)
            if on:
                eu = rows(i, n + b)
                e[b] = _fma32(e[b] - eu, f(scales[b]), eu)
                if factors is not None and factors[i] is not None:
                    e[b] = e[b] * f(factors[i][b])
        x0 = _fma32(x, sa, -(e * s1)) if prediction == "v" else _fma32(-e, s1, x) / sa
        c_x, c_0, _, c_z = (f(c) for c in table[i])
        x = _fma32(x, c_x, x0 * c_0)
        if sigma_noise is not None and c_z != 0.0:
            x = _fma32(sigma_noise[i].astype(f), c_z, x)
        if mask is not None and i + 1 < iters:
            x = blend(x, i + 1)
        latents.append(x.copy())
    return np.stack(latents)


# ------------------------------------------------------------------------------------------------ a trajectory on the CPU

def _guided(od, oc, latent, t, cfg_scale, off, t_range):
    """the noise prediction of one iteration under guidance options, as tests/guidance_ref.py combines the two oracle forwards (base model):
    off: the conditional branch alone; t_range = (t_lo, t_hi): guidance only where t_lo <= t <= t_hi, else e = ec"""
    from oracle.model import unet_forward
    n = latent.shape[0]
    tt = torch.full((n,), t, dtype=torch.int64)
    ec = unet_forward(od.cfg, od.W, latent, tt, oc.context_full, oc.channel_context)
    if off or not (t_range[0] <= t <= t_range[1]):
        return ec
    eu = unet_forward(od.cfg, od.W, latent, tt, oc.unconditional_context_full[None].repeat(n, 1, 1), oc.unconditional_channel_context[None].repeat(n, 1))
    return eu + (ec - eu) * float(cfg_scale)


def cpu_loop(od, pkg, ctx, oc, cfg_scale, ts, table, prediction, seeds, h, w, reference=None, mask=None, latent0=None, renoise_t=None,
             off=False, t_range=None):
    """solver_ref.cpu_solver_loop on a list: the trajectory in fp32 torch on the CPU around the oracle's forward_diffuser, advanced with the
    fp64 rows of `table`; its output is read as `prediction`.  Every noise tensor is fetched from the GPU generator (pkg.gen_noise) under the
    documented draw numbers.  latent0: the latent to refine, re-noised with the DRAW_INITIAL tensor to alphas[renoise_t].  off / t_range:
    the guidance options of _guided."""
    s = schedule(od.alphas, ts)
    assert len(s) == len(table)
    noise = lambda draw: pkg.gen_noise(ctx, seeds, draw, len(seeds), h, w).cpu()
    latent = noise(pkg.DRAW_INITIAL)
    if latent0 is not None:
        a = od.get_alpha(renoise_t)
        latent = latent0 * (a ** 0.5) + latent * ((1.0 - a) ** 0.5)
    x0p = torch.zeros_like(latent)
    for i, (t, a, ap) in enumerate(s):
        if mask is not None:
            latent = torch.where(mask, latent, reference * (a ** 0.5) + noise(pkg.draw_blend(i)) * ((1.0 - a) ** 0.5))
        out = _guided(od, oc, latent, t, cfg_scale, off, t_range) if off or t_range is not None else od.forward_diffuser(latent, t, oc, cfg_scale)
        x0 = latent * (a ** 0.5) - out * ((1.0 - a) ** 0.5) if prediction == "v" else (latent - out * ((1.0 - a) ** 0.5)) / (a ** 0.5)
        c_x, c_0, c_1, c_z = (float(v) for v in table[i])
        latent = latent * c_x + x0 * c_0 + x0p * c_1
        if c_z != 0.0:
            latent = latent + noise(pkg.draw_sigma(i)) * c_z
        x0p = x0
    return latent
