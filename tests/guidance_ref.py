"""fp64 numpy restatement of the guidance options (include/sdxl_mi355.h, sdxl_guidance) and a CPU trajectory loop that applies them.

Per batch entry b and iteration i at timestep t_i, with ec / eu the conditional / unconditional UNet outputs:

    inactive (t_i outside [t_lo, t_hi]):  e = ec
    active:   ecfg = eu + (ec - eu) s_b;  e = ecfg f_b,  f_b = phi r_b + (1 - phi),  r_b = sqrt(M2(ec_b) / M2(ecfg_b))
    off:      e = ec, the unconditional branch is never evaluated

M2 is the centred sum of squares over all values of entry b (CFG rescale, Lin et al. 2023, "Common Diffusion Noise Schedules and Sample
Steps are Flawed", section 3.4: the ratio of standard deviations).  M2(ecfg_b) == 0 gives f_b = 1."""
import numpy as np
import torch

import solver_ref as R
from oracle.model import unet_forward

T_MAX = 2 ** 31 - 1


def rescale_factors(ec, eu, scales, phi):
    """f_b in fp64: ec, eu [n, ...] (any float dtype, widened first), scales [n]"""
    ec, eu = np.asarray(ec, dtype=np.float64), np.asarray(eu, dtype=np.float64)
    n = ec.shape[0]
    ec, eu = ec.reshape(n, -1), eu.reshape(n, -1)
    s = np.asarray(scales, dtype=np.float64).reshape(n, 1)
    ecfg = eu + (ec - eu) * s
    m2 = lambda v: ((v - v.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
    m2c, m2g = m2(ec), m2(ecfg)
    r = np.sqrt(m2c / np.where(m2g == 0.0, 1.0, m2g))
    return np.where(m2g == 0.0, 1.0, phi * r + (1.0 - phi))


def rescale_factors_f32(ec, eu, scales, phi):
    """the same in plain fp32 numpy, two passes (fp32 mean, fp32 centred np.sum): its error against rescale_factors is the yardstick of the
    factors kernel"""
    f = np.float32
    ec, eu = np.asarray(ec, dtype=f), np.asarray(eu, dtype=f)
    n = ec.shape[0]
    ec, eu = ec.reshape(n, -1), eu.reshape(n, -1)
    s = np.asarray(scales, dtype=f).reshape(n, 1)
    ecfg = eu + (ec - eu) * s
    out = np.ones(n, dtype=f)
    for b in range(n):
        m2 = lambda v: np.sum((v - np.mean(v, dtype=f)) ** 2, dtype=f)
        m2c, m2g = m2(ec[b]), m2(ecfg[b])
        if m2g != 0:
            out[b] = f(phi) * np.sqrt(m2c / m2g, dtype=f) + (f(1) - f(phi))
    return out


def active_range(alphas, n_steps, step_start=0):
    """(t_lo, t_hi) covering the middle half of the schedule's iterations"""
    ts = [t for t, _, _ in R.schedule(alphas, n_steps, step_start)]
    return ts[3 * len(ts) // 4 - 1], ts[len(ts) // 4]


def cpu_guided_loop(od, pkg, ctx, oc, cfg_scale, n_steps, seeds, eta, h, w, table, rescale=0.0, scales=None, t_range=None, off=False,
                    reference=None, mask=None):
    """solver_ref.cpu_solver_loop with the two oracle unet_forward calls made separately (base model) and combined in torch fp32 by the rules
    above, the factors in fp64.  Returns (latent, [every f_b used, in order])."""
    s = R.schedule(od.alphas, n_steps)
    assert len(s) == len(table) and not od.is_refiner
    n = len(seeds)
    t_lo, t_hi = t_range if t_range is not None else (0, T_MAX)
    sc = [float(cfg_scale)] * n if scales is None else [float(v) for v in scales]
    noise = lambda draw: pkg.gen_noise(ctx, seeds, draw, n, h, w).cpu()
    latent = noise(pkg.DRAW_INITIAL)
    x0p = torch.zeros_like(latent)
    used = []
    for i, (t, a, ap) in enumerate(s):
        if mask is not None:
            latent = torch.where(mask, latent, reference * (a ** 0.5) + noise(pkg.draw_blend(i)) * ((1.0 - a) ** 0.5))
        ts = torch.full((n,), t, dtype=torch.int64)
        ec = unet_forward(od.cfg, od.W, latent, ts, oc.context_full, oc.channel_context)
        eps = ec
        if not off and t_lo <= t <= t_hi:
            eu = unet_forward(od.cfg, od.W, latent, ts, oc.unconditional_context_full[None].repeat(n, 1, 1),
                              oc.unconditional_channel_context[None].repeat(n, 1))
            eps = eu + (ec - eu) * torch.tensor(sc, dtype=torch.float32).view(n, 1, 1, 1)
            if rescale > 0.0:
                f = rescale_factors(ec.numpy(), eu.numpy(), sc, rescale)
                used.extend(float(v) for v in f)
                eps = eps * torch.from_numpy(f.astype(np.float32)).view(n, 1, 1, 1)
        x0 = (latent - eps * ((1.0 - a) ** 0.5)) / (a ** 0.5)
        c_x, c_0, c_1, c_z = (float(v) for v in table[i])
        latent = latent * c_x + x0 * c_0 + x0p * c_1
        if c_z != 0.0:
            latent = latent + noise(pkg.draw_sigma(i)) * c_z
        x0p = x0
    return latent, used
