"""fp64 numpy restatement of the sampler's coefficient tables (include/sdxl_mi355.h, sdxl_solver_coefficients) and a CPU
trajectory loop around the oracle's forward_diffuser that applies them.

One iteration is x' = c_x x + c_0 x0 + c_1 x0p + c_z z with x0 = (x - sigma e) / alpha the data prediction of this iteration
and x0p the one of the previous iteration.  DPM-Solver++(2M) (Lu et al., "DPM-Solver++: Fast Solver for Guided Sampling of
Diffusion Probabilistic Models", 2022, Algorithm 2) and, for eta > 0, its SDE form (k-diffusion's sample_dpmpp_2m_sde,
midpoint) moved from sigma-space to alpha / sigma:

    alpha = sqrt(a), sigma = sqrt(1 - a), lambda = ln(alpha / sigma), primes for ap, h = lambda' - lambda, r = h_prev / h
    A   = -expm1(-(1 + eta) h)
    c_x = (sigma' / sigma) exp(-eta h)
    c_z = sigma' sqrt(-expm1(-2 eta h))
    second order:  c_0 = alpha' A (1 + 1/(2r)),  c_1 = -alpha' A / (2r)
    first order:   c_0 = alpha' A,               c_1 = 0

First order on iteration 0 and wherever ap == 1 (h infinite: the row is (0, 1, 0, 0) written out)."""
import math

import numpy as np
import torch

DDIM, DPMPP_2M = 0, 1


def schedule(alphas, n_steps, step_start=0):
    """[(t, a, ap)] of `(0..n_train-step_start).rev().step_by(n_train / n_steps)`; ap = 1 where t < step"""
    alphas = np.asarray(alphas, dtype=np.float64)
    n_train = alphas.shape[0]
    step = n_train // n_steps
    return [(t, float(alphas[t]), float(alphas[t - step]) if t >= step else 1.0)
            for t in range(n_train - step_start - 1, -1, -step)]


def ddim_terms(a, ap, eta):
    """(sqrt_ap, sqrt_1map, sigma_t) of the DDIM update x' = x0 sqrt_ap + e sqrt_1map + z sigma_t"""
    sigma_t = 0.0 if eta == 0.0 else eta * math.sqrt((1.0 - ap) / (1.0 - a)) * math.sqrt(1.0 - a / ap)
    return math.sqrt(ap), math.sqrt(max(1.0 - ap - sigma_t * sigma_t, 0.0)), sigma_t


def coefficients(alphas, n_steps, step_start=0, solver=DPMPP_2M, eta=0.0):
    """[iters, 4] float64 rows (c_x, c_0, c_1, c_z)"""
    rows, h_prev = [], None
    for i, (t, a, ap) in enumerate(schedule(alphas, n_steps, step_start)):
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        if solver == DDIM:
            sqrt_ap, sqrt_1map, sigma_t = ddim_terms(a, ap, eta)
            rows.append((sqrt_1map / sigma, sqrt_ap - sqrt_1map * alpha / sigma, 0.0, sigma_t))
            continue
        if ap == 1.0:
            rows.append((0.0, 1.0, 0.0, 0.0))
            h_prev = None
            continue
        alpha_p, sigma_p = math.sqrt(ap), math.sqrt(1.0 - ap)
        h = math.log(alpha_p / sigma_p) - math.log(alpha / sigma)
        A = -math.expm1(-(1.0 + eta) * h)
        c_x = (sigma_p / sigma) * math.exp(-eta * h)
        c_z = sigma_p * math.sqrt(-math.expm1(-2.0 * eta * h))
        if i == 0 or h_prev is None:
            c_0, c_1 = alpha_p * A, 0.0
        else:
            r = h_prev / h
            c_0, c_1 = alpha_p * A * (1.0 + 1.0 / (2.0 * r)), -alpha_p * A / (2.0 * r)
        rows.append((c_x, c_0, c_1, c_z))
        h_prev = h
    return np.array(rows, dtype=np.float64)


def error_gain(table, alphas, n_steps, step_start=0):
    """g = sum_i (|c_0,i| sigma_i / alpha_i + |c_1,i| sigma_{i-1} / alpha_{i-1}): the first-order gain of a UNet-output error
    onto the latent (x0 = (x - sigma e) / alpha carries an error of e scaled by sigma / alpha)"""
    s = schedule(alphas, n_steps, step_start)
    k = [math.sqrt(1.0 - a) / math.sqrt(a) for _, a, _ in s]
    return sum(abs(table[i][1]) * k[i] + (abs(table[i][2]) * k[i - 1] if i else 0.0) for i in range(len(s)))


def analytic_errors(alphas, n_steps, table, var=0.25):
    """Relative error of the state entering the last iteration on Gaussian data N(0, var), whose noise prediction is exact:
    eps(x, t) = sqrt(1 - a) x / (var a + 1 - a), exact state x_t = x_T sqrt((var a_t + 1 - a_t) / (var a_T + 1 - a_T)).
    fp64 loop driven by `table` ((c_x, c_0, c_1, c_z) rows, c_z unused: the ODE)."""
    s = schedule(alphas, n_steps)
    x, x0p = 1.0, 0.0
    for i, (t, a, ap) in enumerate(s[:-1]):
        e = math.sqrt(1.0 - a) * x / (var * a + 1.0 - a)
        x0 = (x - math.sqrt(1.0 - a) * e) / math.sqrt(a)
        c_x, c_0, c_1, _ = table[i]
        x = c_x * x + c_0 * x0 + c_1 * x0p
        x0p = x0
    a_T, a_l = s[0][1], s[-1][1]
    exact = math.sqrt((var * a_l + 1.0 - a_l) / (var * a_T + 1.0 - a_T))
    return abs(x - exact) / exact


def cpu_solver_loop(od, pkg, ctx, oc, cfg_scale, n_steps, seeds, eta, h, w, table, reference=None, mask=None, step_start=0,
                    latent0=None):
    """The trajectory in fp32 torch on the CPU around the oracle's forward_diffuser, advanced with the fp64 rows of `table`;
    every noise tensor is fetched from the GPU generator (pkg.gen_noise) under the draw numbers the engine documents.
    latent0: the latent to refine (re-noised here with the DRAW_INITIAL tensor); None samples from the DRAW_INITIAL tensor."""
    s = schedule(od.alphas, n_steps, step_start)
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
        eps = od.forward_diffuser(latent, t, oc, cfg_scale)
        x0 = (latent - eps * ((1.0 - a) ** 0.5)) / (a ** 0.5)
        c_x, c_0, c_1, c_z = (float(v) for v in table[i])
        latent = latent * c_x + x0 * c_0 + x0p * c_1
        if c_z != 0.0:
            latent = latent + noise(pkg.draw_sigma(i)) * c_z
        x0p = x0
    return latent
