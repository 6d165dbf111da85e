"""fp64 numpy restatement of v-prediction and zero-terminal-SNR schedules in the sampler (include/sdxl_mi355.h, the prediction section),
written from the formulas there and not from the C++.

The network's output is v = alpha e - sigma x0 (alpha = sqrt(a), sigma = sqrt(1 - a), a = alphas_cumprod at the iteration's timestep):

    x0 = alpha x - sigma v            e = alpha v + sigma x

and everything behind x0 and e is the update of tests/solver_ref.py: x' = c_x x + c_0 x0 + c_1 x0p + c_z z, for DDIM x' = sqrt(ap) x0 +
sqrt(1 - ap - sigma_t^2) e + sigma_t z.  The rows do not depend on the prediction type.  A zero-terminal-SNR table has a == 0 on iteration 0:
alpha = 0, sigma = 1, lambda = ln(alpha / sigma) = -inf, h = lambda' - lambda = +inf.  DDIM's terms are finite there as they stand (sigma_t =
eta sqrt(1 - ap)).  For DPM-Solver++(2M) the limits of the first-order row are A = -expm1(-(1 + eta) h) -> 1, so c_0 = alpha'; c_x =
(sigma' / sigma) exp(-eta h) -> sigma' at eta == 0 and 0 at eta > 0; c_z = sigma' sqrt(-expm1(-2 eta h)) -> 0 at eta == 0 and sigma' at
eta > 0.  The iteration behind such a row has r = h_prev / h = inf: 1 / (2r) = 0, first order, the history is not consulted."""
import math

import numpy as np
import torch

import solver_ref as R

DDIM, DPMPP_2M = R.DDIM, R.DPMPP_2M
U = 2.0 ** -24          # half an ulp of 1.0 in fp32: the relative error of one rounding


def rescale_zero_terminal_snr(alphas):
    """Lin et al. 2023, Algorithm 1 on s = sqrt(alphas_cumprod) in f64 -> (s * s as float64, the same cast to float32)"""
    s = np.sqrt(np.asarray(alphas, dtype=np.float32).astype(np.float64))
    s0, sT = s[0], s[-1]
    s = (s - sT) * s0 / (s0 - sT)
    return s * s, (s * s).astype(np.float32)


def coefficients(alphas, n_steps, step_start=0, solver=DPMPP_2M, eta=0.0):
    """[iters, 4] float64 rows (c_x, c_0, c_1, c_z), a == 0 admitted on an iteration"""
    rows, h_prev = [], None
    for t, a, ap in R.schedule(alphas, n_steps, step_start):
        assert 0.0 <= a < 1.0 and 0.0 < ap <= 1.0
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        if solver == DDIM:
            sqrt_ap, sqrt_1map, sigma_t = R.ddim_terms(a, ap, eta)
            rows.append((sqrt_1map / sigma, sqrt_ap - sqrt_1map * alpha / sigma, 0.0, sigma_t))
            continue
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
        c_x = (sigma_p / sigma) * math.exp(-eta * h)
        c_z = sigma_p * math.sqrt(-math.expm1(-2.0 * eta * h))
        if h_prev is None:
            c_0, c_1 = alpha_p * A, 0.0
        else:
            r = h_prev / h
            c_0, c_1 = alpha_p * A * (1.0 + 1.0 / (2.0 * r)), -alpha_p * A / (2.0 * r)
        rows.append((c_x, c_0, c_1, c_z))
        h_prev = h
    return np.array(rows, dtype=np.float64)


def error_gain_v(table, alphas, n_steps, step_start=0):
    """g_v = sum_i (|c_0,i| sigma_i + |c_1,i| sigma_{i-1}): the first-order gain of a UNet-output error onto the latent under v, where
    x0 = alpha x - sigma v carries an error of v scaled by sigma (no 1 / alpha)"""
    k = [math.sqrt(1.0 - a) for _, a, _ in R.schedule(alphas, n_steps, step_start)]
    return sum(abs(table[i][1]) * k[i] + (abs(table[i][2]) * k[i - 1] if i else 0.0) for i in range(len(k)))


def _f32(x):
    return float(np.float32(x))


def replay(alphas, n_steps, step_start, solver, eta, v_rows, latent0, scales=None, active=None, factors=None, reference=None, mask=None,
           blend_noise=None, sigma_noise=None):
    """The per-step arithmetic in fp64 on what the device holds: per iteration the table row rounded to fp32 and sqrt_a, sqrt_1ma rounded to
    fp32.  All arrays float64 numpy.  v_rows [iters, B, HW, 4] (B = n: one branch; B = 2n: cond entries first); latent0 [n, 4, h, w];
    scales [n] (None: one branch); active [iters] bools (None: every iteration); factors [iters][n] or None (CFG rescale, None entries on
    inactive iterations); reference / mask [n, 4, h, w] with blend_noise [iters, n, 4, h, w] (inpainting: mask True keeps the generated
    value); sigma_noise [iters, n, 4, h, w] or None (the z of iteration i, used where its coefficient != 0).
    Returns (latents [iters + 1, n, 4, h, w], last x0, M [iters + 1]): M[i] the largest value, over the updates in front of recorded
    latent i, of |c_x x| + |c_0 x0| + |c_1 x0p| + |c_z z| (DDIM: |sqrt_ap x0| + |sqrt_1map e| + |sigma_t z|); M[0] is the size of the
    step-0 blend terms |ref sqrt_a| + |z sqrt_1ma| under inpainting (the only arithmetic in front of latent 0) and 0 without."""
    s = R.schedule(alphas, n_steps, step_start)
    iters = len(s)
    table = coefficients(alphas, n_steps, step_start, solver, eta)
    n, _, h, w = latent0.shape
    x = latent0.astype(np.float64).copy()
    x0p = np.zeros_like(x)
    rows = lambda i, b: v_rows[i, b].reshape(h, w, 4).transpose(2, 0, 1)      # [HW, 4] -> [4, h, w]

    def blend(x, i):
        sa, s1 = _f32(math.sqrt(s[i][1])), _f32(math.sqrt(1.0 - s[i][1]))
        return np.where(mask, x, reference * sa + blend_noise[i] * s1), float((np.abs(reference * sa) + np.abs(blend_noise[i] * s1)).max())

    M, m = [0.0], 0.0
    if mask is not None:
        x, M[0] = blend(x, 0)
    latents, x0 = [x.copy()], None
    for i, (t, a, ap) in enumerate(s):
        sa, s1 = _f32(math.sqrt(a)), _f32(math.sqrt(1.0 - a))
        on = scales is not None and (active is None or bool(active[i]))
        v = np.empty_like(x)
        for b in range(n):
            v[b] = rows(i, b)
            if on:
                vu = rows(i, n + b)
                v[b] = vu + (v[b] - vu) * _f32(scales[b])
                if factors is not None and factors[i] is not None:
                    v[b] = v[b] * float(factors[i][b])
        x0 = x * sa - v * s1
        z = sigma_noise[i] if sigma_noise is not None else None
        if solver == DDIM:
            sqrt_ap, sqrt_1map, sigma_t = (_f32(c) for c in R.ddim_terms(a, ap, eta))
            e = v * sa + x * s1
            terms = np.abs(x0 * sqrt_ap) + np.abs(e * sqrt_1map)
            x = x0 * sqrt_ap + e * sqrt_1map
            cz = sigma_t
        else:
            c_x, c_0, c_1, cz = (_f32(c) for c in table[i])
            terms = np.abs(x * c_x) + np.abs(x0 * c_0) + np.abs(x0p * c_1)
            x = x * c_x + x0 * c_0 + x0p * c_1
        if z is not None and cz != 0.0:
            terms = terms + np.abs(z * cz)
            x = x + z * cz
        x0p = x0
        m = max(m, float(terms.max()))
        if mask is not None and i + 1 < iters:
            x, _ = blend(x, i + 1)
        latents.append(x.copy())
        M.append(m)
    return np.stack(latents), x0, np.array(M)


def cpu_v_loop(od, pkg, ctx, oc, cfg_scale, n_steps, seeds, eta, h, w, table, reference=None, mask=None, step_start=0, latent0=None):
    """solver_ref.cpu_solver_loop with the oracle's forward_diffuser output read as v: x0 = alpha x - sigma v, then the fp64 rows of `table`
    (DDIM's folded into the same four numbers).  Noise from the GPU generator under the documented draw numbers."""
    s = R.schedule(od.alphas, n_steps, step_start)
    assert len(s) == len(table)
    noise = lambda draw: pkg.gen_noise(ctx, seeds, draw, len(seeds), h, w).cpu()
    latent = noise(pkg.DRAW_INITIAL)
    if latent0 is not None:
        a = od.get_alpha(od.n_steps - step_start)
        latent = latent0 * (a ** 0.5) + latent * ((1.0 - a) ** 0.5)
    x0p = torch.zeros_like(latent)
    for i, (t, a, ap) in enumerate(s):
        if mask is not None:
            latent = torch.where(mask, latent, reference * (a ** 0.5) + noise(pkg.draw_blend(i)) * ((1.0 - a) ** 0.5))
        v = od.forward_diffuser(latent, t, oc, cfg_scale)
        x0 = latent * (a ** 0.5) - v * ((1.0 - a) ** 0.5)
        c_x, c_0, c_1, c_z = (float(c) for c in table[i])
        latent = latent * c_x + x0 * c_0 + x0p * c_1
        if c_z != 0.0:
            latent = latent + noise(pkg.draw_sigma(i)) * c_z
        x0p = x0
    return latent
