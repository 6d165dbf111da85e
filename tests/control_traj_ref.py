"""CPU reference of a sampling trajectory with control nets, and a Python restatement of the scale table (sdxl_control_scale_table).  The engine's
Diffuser does not take a control net yet: the loop is the reference a test of that wiring compares against, and
tests/test_cpu_control_trajectory.py holds the fixture it gives to "it matters and behaves".

The loop is guidance_ref.cpu_guided_loop's -- the two branches of an iteration evaluated separately in fp32 torch and combined by the rules there,
the update from the fp64 rows of solver_ref.coefficients -- with each branch's noise prediction

    e = controlled_unet_forward(x, t, context, label, residuals = sum_k s_k(i, b) control_forward_k(x, t, context, label, hint_k))

(tests/controlnet_ref.py), b the batch entry of the row: b = j for the conditional branch of image j, n + j for the unconditional one, whose hint
is image j's.  The residuals are summed in fp64 and handed on as fp32; a net all of whose scales are 0 on a branch of an iteration is not evaluated.

    s_k(i, b) = (t_lo <= t_i <= t_hi) ? (scales ? scales[b mod n] : scale) : 0,   and 0 for b >= n under cond_only      (include/sdxl_mi355.h)
"""
import numpy as np
import torch

import controlnet_ref as CR
import solver_ref as R

T_MAX = 2 ** 31 - 1


def scale_table(n, timesteps, single=False, scale=1.0, scales=None, t_range=None, cond_only=False):
    """float32 [len(timesteps) + 1, 8]: row i = s(i, .) over the B = n (single) or 2 n batch entries, zeros behind them; the last row zeros"""
    B = n if single else 2 * n
    lo, hi = t_range if t_range is not None else (0, T_MAX)
    out = np.zeros((len(timesteps) + 1, 8), dtype=np.float32)
    for i, t in enumerate(timesteps):
        if not lo <= t <= hi:
            continue
        for b in range(B):
            if cond_only and b >= n:
                continue
            out[i, b] = scales[b % n] if scales else scale
    return out


def cpu_controlled_loop(ocfg, W, alphas, oc, cfg_scale, n_steps, n, table, noise, controls, off=False, guidance_scales=None, reference=None,
                        mask=None, step_start=0, latent0=None, trace=None):
    """controls: [dict(W=control weights, hint=[n, 3, H8, W8], options=dict of scale_table's keywords)], any number.
    noise(key): the noise tensor [n, 4, h, w] of key ("initial",), ("blend", i) or ("sigma", i) -- the draws the engine documents.
    off: the conditional branch alone (SDXL_GUIDANCE_OFF).  latent0 / step_start: refine.  trace: a list that receives the latent after every
    iteration.  Returns the final latent."""
    s = R.schedule(alphas, n_steps, step_start)
    assert len(s) == len(table)
    tabs = [scale_table(n, [t for t, _, _ in s], single=off, **c["options"]) for c in controls]
    sc = [float(cfg_scale)] * n if guidance_scales is None else [float(v) for v in guidance_scales]
    latent = noise(("initial",))
    if latent0 is not None:
        a = float(np.asarray(alphas, dtype=np.float64)[len(alphas) - step_start])
        latent = latent0 * (a ** 0.5) + latent * ((1.0 - a) ** 0.5)
    x0p = torch.zeros_like(latent)
    for i, (t, a, ap) in enumerate(s):
        if mask is not None:
            latent = torch.where(mask, latent, reference * (a ** 0.5) + noise(("blend", i)) * ((1.0 - a) ** 0.5))
        ts = torch.full((n,), t, dtype=torch.int64)

        def branch(context, label, first):
            total = None
            for c, tab in zip(controls, tabs):
                sk = tab[i, first:first + n].astype(np.float64)
                if not sk.any():
                    continue
                r = CR.control_forward(ocfg, c["W"], latent, ts, context, label, c["hint"])
                r = [x.double() * torch.from_numpy(sk).view(n, 1, 1, 1) for x in r]
                total = r if total is None else [p + q for p, q in zip(total, r)]
            return CR.controlled_unet_forward(ocfg, W, latent, ts, context, label, None if total is None else [x.float() for x in total], 1.0)

        eps = branch(oc.context_full, oc.channel_context, 0)
        if not off:
            eu = branch(oc.unconditional_context_full[None].repeat(n, 1, 1), oc.unconditional_channel_context[None].repeat(n, 1), n)
            eps = eu + (eps - eu) * torch.tensor(sc, dtype=torch.float32).view(n, 1, 1, 1)
        x0 = (latent - eps * ((1.0 - a) ** 0.5)) / (a ** 0.5)
        c_x, c_0, c_1, c_z = (float(v) for v in table[i])
        latent = latent * c_x + x0 * c_0 + x0p * c_1
        if c_z != 0.0:
            latent = latent + noise(("sigma", i)) * c_z
        x0p = x0
        if trace is not None:
            trace.append(latent.clone())
    return latent


def first_non_finite(trace, n):
    """(iteration, batch entry) of the first non-finite latent of a trace [iters, n, ...], or None"""
    for i in range(trace.shape[0]):
        for b in range(n):
            if not bool(torch.isfinite(trace[i, b]).all()):
                return i, b
    return None
