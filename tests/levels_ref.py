"""fp64 restatement of the noise-level schedules (include/sdxl_mi355.h, the noise-level section), written from the formulas there and from
k-diffusion's published loops, not from the C++: sigma_to_t, the three sigma spacings, a schedule as [(t, a, ap)] from a timestep list
with an end timestep or a sigma list with an end sigma, the five-column rows (c_x, c_0, c_1, c_2, c_z) of every solver on such a schedule
-- the DPM++ 3M SDE rows twice, from the alpha / sigma formulas and from the literal variance-exploding loop --, an fp64 replay and an fp32
emulation of the per-step arithmetic with both histories, and a CPU trajectory loop that feeds the oracle's UNet a float timestep.

One iteration is x' = c_x x + c_0 x0 + c_1 x0p + c_2 x0pp + c_z z; alpha = sqrt(a), sigma = sqrt(1 - a), primes for ap; k-diffusion's
sigma is sigma / alpha."""
import math

import numpy as np
import torch

import solver_ref as R

DDIM, DPMPP_2M, LCM, TCD, DPMPP_3M = 0, 1, 3, 4, 5
SOLVERS = {"ddim": DDIM, "dpmpp_2m": DPMPP_2M, "lcm": LCM, "tcd": TCD, "dpmpp_3m": DPMPP_3M}
U = 2.0 ** -24          # half an ulp of 1.0 in fp32: the relative error of one rounding


def _alphas64(alphas):
    return np.asarray(alphas, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ sigmas

def sigma_of(a):
    return math.sqrt((1.0 - a) / a)


def sigma_to_t(alphas, sigma, round_t=False):
    """k-diffusion's DiscreteSchedule.sigma_to_t (quantize = False) in f64"""
    al = _alphas64(alphas)
    L = 0.5 * np.log((1.0 - al) / al)
    ls = math.log(sigma)
    below = np.nonzero(L[:-1] <= ls)[0]
    low = int(below[-1]) if len(below) else 0
    high = low + 1
    w = (L[low] - ls) / (L[low] - L[high])
    w = min(max(w, 0.0), 1.0)
    t = (1.0 - w) * low + w * high
    return float(np.rint(t)) if round_t else float(t)


def table_ends(alphas):
    al = _alphas64(alphas)
    return sigma_of(al[0]), sigma_of(al[-1])


def sigmas_karras(n, alphas, sigma_min=0.0, sigma_max=0.0, rho=7.0):
    """k-diffusion's get_sigmas_karras without the appended 0"""
    lo, hi = table_ends(alphas)
    lo, hi = (sigma_min if sigma_min > 0 else lo), (sigma_max if sigma_max > 0 else hi)
    ramp = [0.0] if n == 1 else [i / (n - 1) for i in range(n)]
    return [(hi ** (1.0 / rho) + r * (lo ** (1.0 / rho) - hi ** (1.0 / rho))) ** rho for r in ramp]


def sigmas_exponential(n, alphas, sigma_min=0.0, sigma_max=0.0):
    """k-diffusion's get_sigmas_exponential without the appended 0"""
    lo, hi = table_ends(alphas)
    lo, hi = (sigma_min if sigma_min > 0 else lo), (sigma_max if sigma_max > 0 else hi)
    ramp = [0.0] if n == 1 else [i / (n - 1) for i in range(n)]
    return [math.exp(math.log(hi) + r * (math.log(lo) - math.log(hi))) for r in ramp]


def sigmas_of_timesteps(n_steps, alphas):
    al = _alphas64(alphas)
    n_train = len(al)
    return [sigma_of(float(al[t])) for t in range(n_train - 1, -1, -(n_train // n_steps))]


# ------------------------------------------------------------------------------------------------ schedules

def levels(alphas, timesteps=None, sigmas=None, t_end=-1, sigma_end=0.0, round_t=False):
    """[(t, a, ap)] of a timestep list with an end timestep (-1: ap = 1) or of a sigma list with an end sigma (0: ap = 1); t is a float"""
    al = _alphas64(alphas)
    assert (timesteps is None) != (sigmas is None)
    if timesteps is not None:
        ts = [int(t) for t in timesteps]
        assert all(0 <= t < len(al) for t in ts) and all(b < a for a, b in zip(ts, ts[1:])) and -1 <= t_end < ts[-1]
        t, a, a_end = [float(v) for v in ts], [float(al[v]) for v in ts], 1.0 if t_end < 0 else float(al[t_end])
    else:
        sg = [float(s) for s in sigmas]
        assert all(s > 0 and math.isfinite(s) for s in sg) and all(b < a for a, b in zip(sg, sg[1:])) and 0.0 <= sigma_end < sg[-1]
        t, a = [sigma_to_t(alphas, s, round_t) for s in sg], [1.0 / (1.0 + s * s) for s in sg]
        a_end = 1.0 if sigma_end == 0.0 else 1.0 / (1.0 + sigma_end * sigma_end)
    return [(t[i], a[i], a[i + 1] if i + 1 < len(a) else a_end) for i in range(len(a))]


# ------------------------------------------------------------------------------------------------ rows

def _limit_row(ap, eta):
    """a == 0 under v-prediction: h = +inf, the limits 2M takes"""
    alpha_p, sigma_p = math.sqrt(ap), math.sqrt(1.0 - ap)
    return (sigma_p, alpha_p, 0.0, 0.0, 0.0) if eta == 0.0 else (0.0, alpha_p, 0.0, 0.0, sigma_p)


def rows_3m_vp(lv, eta=0.0):
    """the DPM++ 3M SDE rows from the alpha / sigma formulas of the public header"""
    rows, hs = [], []            # hs: the h of the previous iterations since the order last restarted, newest first
    for t, a, ap in lv:
        if ap == 1.0:
            rows.append((0.0, 1.0, 0.0, 0.0, 0.0))
            hs = []
            continue
        if a == 0.0:
            rows.append(_limit_row(ap, eta))
            hs = []
            continue
        alpha, sigma, alpha_p, sigma_p = math.sqrt(a), math.sqrt(1.0 - a), math.sqrt(ap), math.sqrt(1.0 - ap)
        h = math.log(alpha_p / sigma_p) - math.log(alpha / sigma)
        he = (1.0 + eta) * h
        A = -math.expm1(-he)
        phi2 = math.expm1(-he) / he + 1.0
        phi3 = phi2 / he - 0.5
        c_x, c_z = (sigma_p / sigma) * math.exp(-eta * h), sigma_p * math.sqrt(-math.expm1(-2.0 * eta * h))
        if len(hs) >= 2:
            r0, r1 = hs[0] / h, hs[1] / h
            P = phi2 * (1.0 + r0 / (r0 + r1)) - phi3 / (r0 + r1)
            Q = (phi3 - phi2 * r0) / (r0 + r1)
            c = (alpha_p * (A + P / r0), alpha_p * (-P / r0 + Q / r1), -alpha_p * Q / r1)
        elif len(hs) == 1:
            r0 = hs[0] / h
            c = (alpha_p * (A + phi2 / r0), -alpha_p * phi2 / r0, 0.0)
        else:
            c = (alpha_p * A, 0.0, 0.0)
        rows.append((c_x, c[0], c[1], c[2], c_z))
        hs = [h] + hs[:1]
    return np.array(rows, dtype=np.float64)


def _ve_step(x, den, den1, den2, noise, sig, sig_next, eta, h_1, h_2):
    """one iteration of k-diffusion's sample_dpmpp_3m_sde, line by line, in its own (variance-exploding) variables; s_noise = 1.
    Returns (x', h)"""
    if sig_next == 0:
        return den, None
    t, s = -math.log(sig), -math.log(sig_next)
    h = s - t
    h_eta = h * (eta + 1)
    x = math.exp(-h_eta) * x + (-math.expm1(-h_eta)) * den
    if h_2 is not None:
        r0 = h_1 / h
        r1 = h_2 / h
        d1_0 = (den - den1) / r0
        d1_1 = (den1 - den2) / r1
        d1 = d1_0 + (d1_0 - d1_1) * r0 / (r0 + r1)
        d2 = (d1_0 - d1_1) / (r0 + r1)
        phi_2 = math.expm1(-h_eta) / h_eta + 1
        phi_3 = phi_2 / h_eta - 0.5
        x = x + phi_2 * d1 - phi_3 * d2
    elif h_1 is not None:
        r = h_1 / h
        d = (den - den1) / r
        phi_2 = math.expm1(-h_eta) / h_eta + 1
        x = x + phi_2 * d
    if eta:
        x = x + noise * sig_next * math.sqrt(-math.expm1(-2 * h * eta))
    return x, h


def rows_3m_ve(lv, eta=0.0):
    """the same rows read off the literal loop: the update is linear in (x, denoised, denoised_1, denoised_2, noise), so one evaluation
    per unit vector gives its five coefficients in k-diffusion's variables x_ve = x / alpha, sigma_ve = sigma / alpha; x' = alpha' x_ve'
    turns them into the rows.  Needs a > 0 everywhere (sigma_ve is infinite at a == 0)."""
    rows, h_1, h_2 = [], None, None
    for t, a, ap in lv:
        alpha, alpha_p = math.sqrt(a), math.sqrt(ap)
        sig, sig_next = math.sqrt(1.0 - a) / alpha, math.sqrt(1.0 - ap) / alpha_p
        unit = lambda k: _ve_step(*[1.0 if j == k else 0.0 for j in range(5)], sig, sig_next, eta, h_1, h_2)[0]
        h = _ve_step(0.0, 0.0, 0.0, 0.0, 0.0, sig, sig_next, eta, h_1, h_2)[1]
        rows.append((alpha_p * unit(0) / alpha, alpha_p * unit(1), alpha_p * unit(2), alpha_p * unit(3), alpha_p * unit(4)))
        if h is None:
            h_1, h_2 = None, None      # (the loop ends here in k-diffusion; the engine restarts the order behind such a row)
        else:
            h_1, h_2 = h, h_1
    return np.array(rows, dtype=np.float64)


def rows_ddim(lv, eta=0.0):
    rows = []
    for t, a, ap in lv:
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        sqrt_ap, sqrt_1map, sigma_t = R.ddim_terms(a, ap, eta)
        rows.append((sqrt_1map / sigma, sqrt_ap - sqrt_1map * alpha / sigma, 0.0, 0.0, sigma_t))
    return np.array(rows, dtype=np.float64)


def rows_2m(lv, eta=0.0):
    rows, h_prev = [], None
    for t, a, ap in lv:
        if ap == 1.0:
            rows.append((0.0, 1.0, 0.0, 0.0, 0.0))
            h_prev = None
            continue
        if a == 0.0:
            rows.append(_limit_row(ap, eta))
            h_prev = None
            continue
        alpha, sigma, alpha_p, sigma_p = math.sqrt(a), math.sqrt(1.0 - a), math.sqrt(ap), math.sqrt(1.0 - ap)
        h = math.log(alpha_p / sigma_p) - math.log(alpha / sigma)
        A = -math.expm1(-(1.0 + eta) * h)
        c_x, c_z = (sigma_p / sigma) * math.exp(-eta * h), sigma_p * math.sqrt(-math.expm1(-2.0 * eta * h))
        if h_prev is None:
            c_0, c_1 = alpha_p * A, 0.0
        else:
            r = h_prev / h
            c_0, c_1 = alpha_p * A * (1.0 + 1.0 / (2.0 * r)), -alpha_p * A / (2.0 * r)
        rows.append((c_x, c_0, c_1, 0.0, c_z))
        h_prev = h
    return np.array(rows, dtype=np.float64)


def rows_lcm(lv):
    rows = []
    for t, a, ap in lv:
        s = 10.0 * t
        c_skip, c_out = 0.25 / (s * s + 0.25), s / math.sqrt(s * s + 0.25)
        rows.append((math.sqrt(ap) * c_skip, math.sqrt(ap) * c_out, 0.0, 0.0, math.sqrt(1.0 - ap)))
    return np.array(rows, dtype=np.float64)


def coefficients(lv, solver, eta=0.0):
    """[len(lv), 5] float64 rows of a solver (not TCD: it reads training timesteps, tests/fewstep_ref.py has it)"""
    solver = SOLVERS.get(solver, solver)
    if solver == LCM:
        assert eta == 0.0
        return rows_lcm(lv)
    return {DDIM: rows_ddim, DPMPP_2M: rows_2m, DPMPP_3M: rows_3m_vp}[solver](lv, eta)


def error_gain(table, lv, prediction="epsilon"):
    """the first-order gain of a UNet-output error onto the latent, sum_i (|c_0,i| k_i + |c_1,i| k_{i-1} + |c_2,i| k_{i-2}), k = sigma / alpha
    under epsilon and sigma under v: tests/fewstep_ref.py error_gain with the second history term"""
    k = [math.sqrt(1.0 - a) / (math.sqrt(a) if prediction == "epsilon" else 1.0) for _, a, _ in lv]
    return sum(abs(table[i][1]) * k[i] + (abs(table[i][2]) * k[i - 1] if i >= 1 else 0.0) + (abs(table[i][3]) * k[i - 2] if i >= 2 else 0.0)
               for i in range(len(k)))


# ------------------------------------------------------------------------------------------------ the per-step arithmetic

def _f32(x):
    return float(np.float32(x))


def _guided(rows, i, n, scales, on, factors, f=None):
    """the guidance lines of iteration i -> [n, 4, h, w]; f: None for fp64, else the fp32 emulation's rounding"""
    e = [rows(i, b) for b in range(n)]
    for b in range(n):
        if on:
            eu = rows(i, n + b)
            e[b] = eu + (e[b] - eu) * _f32(scales[b]) if f is None else _fma32((e[b] - eu).astype(f), f(scales[b]), eu)
            if factors is not None and factors[i] is not None:
                e[b] = e[b] * (float(factors[i][b]) if f is None else f(factors[i][b]))
    return np.stack(e)


def replay(lv, solver, table, rows_in, latent0, prediction="epsilon", scales=None, active=None, factors=None, reference=None, mask=None,
           blend_noise=None, sigma_noise=None):
    """tests/fewstep_ref.py replay for every solver on a schedule lv, with the c_2 / second-history terms: fp64 arithmetic on what the device
    holds (the table row -- under DDIM sqrt_ap, sqrt_1map, sigma_t --, sqrt_a and sqrt_1ma rounded to fp32).  Arguments as there.
    Returns (latents [iters + 1, n, 4, h, w], M [iters + 1], hist, hist2).  M[i]: the largest |c_x x| + |c_0 x0| + |c_1 x0p| + |c_2 x0pp| +
    |c_z z| (DDIM: |sqrt_ap x0| + |sqrt_1map e| + |sigma_t z|) over the updates in front of recorded latent i; M[0] the step-0 blend terms.
    hist / hist2: the two history buffers after the last update by the kernel's rule -- hist = x0 on every update, hist2 = x0p on the
    updates whose c_1 != 0 (None while never written)."""
    solver = SOLVERS.get(solver, solver)
    iters = len(lv)
    assert len(table) == iters
    n, _, h, w = latent0.shape
    x = latent0.astype(np.float64).copy()
    rows = lambda i, b: rows_in[i, b].reshape(h, w, 4).transpose(2, 0, 1).astype(np.float64)

    def blend(x, i):
        sa, s1 = _f32(math.sqrt(lv[i][1])), _f32(math.sqrt(1.0 - lv[i][1]))
        return np.where(mask, x, reference * sa + blend_noise[i] * s1), float((np.abs(reference * sa) + np.abs(blend_noise[i] * s1)).max())

    M, m = [0.0], 0.0
    if mask is not None:
        x, M[0] = blend(x, 0)
    latents, hist, hist2 = [x.copy()], None, None
    for i, (t, a, ap) in enumerate(lv):
        sa, s1 = _f32(math.sqrt(a)), _f32(math.sqrt(1.0 - a))
        on = scales is not None and (active is None or bool(active[i]))
        e = _guided(rows, i, n, scales, on, factors)
        x0 = x * sa - e * s1 if prediction == "v" else (x - e * s1) / sa
        c_x, c_0, c_1, c_2, c_z = (_f32(c) for c in table[i])
        if solver == DDIM:
            sqrt_ap, sqrt_1map, c_z = (_f32(c) for c in _ddim_device_terms(ap, table[i][4]))
            if prediction == "v":
                e = e * sa + x * s1
            terms = np.abs(x0 * sqrt_ap) + np.abs(e * sqrt_1map)
            x = x0 * sqrt_ap + e * sqrt_1map
        else:
            x0p = hist if c_1 != 0.0 else 0.0
            x0pp = hist2 if c_2 != 0.0 else 0.0
            terms = np.abs(x * c_x) + np.abs(x0 * c_0) + np.abs(x0p * c_1) + np.abs(x0pp * c_2)
            x = x * c_x + x0 * c_0 + x0p * c_1 + x0pp * c_2
            if c_1 != 0.0:
                hist2 = hist
            hist = x0
        if sigma_noise is not None and c_z != 0.0:
            terms = terms + np.abs(sigma_noise[i] * c_z)
            x = x + sigma_noise[i] * c_z
        m = max(m, float(terms.max()))
        if mask is not None and i + 1 < iters:
            x, _ = blend(x, i + 1)
        latents.append(x.copy())
        M.append(m)
    return np.stack(latents), np.array(M), hist, hist2


def x0_with_bound(lv, i, x, rows_in, prediction="epsilon", scales=None, active=None, factors=None):
    """(x0, tol) of iteration i in fp64 from the latent x in front of it (as the device recorded it, blend included) and the network's rows.
    tol: the x0 the kernel computes from the same fp32 x is at most six roundings away -- the difference and the fma of the guidance line, the
    rescale product, under v the product v sqrt_1ma, the fma, under epsilon the quotient --, each at most half an ulp of a value no larger
    than T = (|x| + (|ec - eu| |s| + |eu| + |e|) sqrt_1ma) / sqrt_a  (v: |x| sqrt_a + (...) sqrt_1ma)"""
    n, _, h, w = x.shape
    rows = lambda j, b: rows_in[j, b].reshape(h, w, 4).transpose(2, 0, 1).astype(np.float64)
    t, a, ap = lv[i]
    sa, s1 = _f32(math.sqrt(a)), _f32(math.sqrt(1.0 - a))
    on = scales is not None and (active is None or bool(active[i]))
    e = _guided(rows, i, n, scales, on, factors)
    size = np.abs(e)
    if on:
        size = size + np.stack([np.abs(rows(i, b) - rows(i, n + b)) * abs(_f32(scales[b])) + np.abs(rows(i, n + b)) for b in range(n)])
    if prediction == "v":
        return x * sa - e * s1, 6 * U * float((np.abs(x) * sa + size * s1).max())
    return (x - e * s1) / sa, 6 * U * float(((np.abs(x) + size * s1) / sa).max())


def _ddim_device_terms(ap, sigma_t):
    """(sqrt_ap, sqrt_1map, sigma_t): the three update terms the DDIM layout of the device table holds, from the row's c_z = sigma_t"""
    return math.sqrt(ap), math.sqrt(max(1.0 - ap - sigma_t * sigma_t, 0.0)), sigma_t


def _fma32(a, b, c):
    """fp32 fma of fp32 arrays: the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double
    rounding differs from the fused one in about one case in 2^29: nothing a bound with a margin notices)"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def emulate_f32(lv, solver, table, rows_in, latent0, prediction="epsilon", scales=None, active=None, factors=None, reference=None, mask=None,
                blend_noise=None, sigma_noise=None):
    """the lines of the per-step kernel in fp32 numpy, rounding by rounding as the header states them, for every solver:
    e = fma(ec - eu, s_b, eu) (* f_b);  x0 = fma(-e, sqrt_1ma, x) / sqrt_a  or  fma(x, sqrt_a, -(v sqrt_1ma));
    3M / 2M / first-order rows: acc = c_2 x0pp;  acc = fma(x0p, c_1, acc);  acc = fma(x0, c_0, acc);  x = fma(x, c_x, acc) -- 2M starts at
    acc = c_1 x0p, a first-order row at acc = x0 c_0 (adding the exact zeros of the absent terms changes no bit but the sign of a zero);
    DDIM: e = fma(v, sqrt_a, x sqrt_1ma) under v, x = x0 sqrt_ap + e sqrt_1map with both products rounded on channels 0 and 1 and the
    first one fused on channels 2 and 3;  x = fma(z, c_z, x);  the blend rounds both products.  Returns latents float32 [iters + 1, ...]"""
    f = np.float32
    solver = SOLVERS.get(solver, solver)
    iters = len(lv)
    n, _, h, w = latent0.shape
    x = latent0.astype(f).copy()
    rows = lambda i, b: rows_in[i, b].reshape(h, w, 4).transpose(2, 0, 1).astype(f)

    def blend(x, i):
        sa, s1 = f(math.sqrt(lv[i][1])), f(math.sqrt(1.0 - lv[i][1]))
        return np.where(mask, x, (reference.astype(f) * sa + blend_noise[i].astype(f) * s1).astype(f))

    if mask is not None:
        x = blend(x, 0)
    latents = [x.copy()]
    hist, hist2 = np.zeros_like(x), np.zeros_like(x)
    for i, (t, a, ap) in enumerate(lv):
        sa, s1 = f(math.sqrt(a)), f(math.sqrt(1.0 - a))
        on = scales is not None and (active is None or bool(active[i]))
        e = _guided(rows, i, n, scales, on, factors, f).astype(f)
        x0 = _fma32(x, sa, -(e * s1)) if prediction == "v" else _fma32(-e, s1, x) / sa
        c_x, c_0, c_1, c_2, c_z = (f(c) for c in table[i])
        if solver == DDIM:
            sqrt_ap, sqrt_1map, c_z = (f(c) for c in _ddim_device_terms(ap, table[i][4]))
            if prediction == "v":
                e = _fma32(e, sa, x * s1)
            en = e * sqrt_1map
            x = np.concatenate([x0[:, :2] * sqrt_ap + en[:, :2], _fma32(x0[:, 2:], sqrt_ap, en[:, 2:])], axis=1)
        else:
            x0p = hist if c_1 != 0 else np.zeros_like(x)
            x0pp = hist2 if c_2 != 0 else np.zeros_like(x)
            acc = c_2 * x0pp
            acc = _fma32(x0p, c_1, acc)
            acc = _fma32(x0, c_0, acc)
            x = _fma32(x, c_x, acc)
            if c_1 != 0:
                hist2 = hist
            hist = x0
        if sigma_noise is not None and c_z != 0.0:
            x = _fma32(sigma_noise[i].astype(f), c_z, x)
        if mask is not None and i + 1 < iters:
            x = blend(x, i + 1)
        latents.append(x.copy())
    return np.stack(latents)


# ------------------------------------------------------------------------------------------------ a trajectory on the CPU

def unet_eps(od, oc, latent, t, cfg_scale, refiner=False):
    """the CFG-combined output of the oracle's UNet at a float timestep t (oracle/pipeline.py forward_diffuser takes an int): the refiner's
    conditional branch alone, as the reference runs it"""
    from oracle.model import unet_forward
    n = latent.shape[0]
    tt = torch.full((n,), float(np.float32(t)), dtype=torch.float32)
    if refiner:
        return unet_forward(od.cfg, od.W, latent, tt, oc.context_open_clip, oc.channel_context_refiner)
    ec = unet_forward(od.cfg, od.W, latent, tt, oc.context_full, oc.channel_context)
    eu = unet_forward(od.cfg, od.W, latent, tt, oc.unconditional_context_full[None].repeat(n, 1, 1), oc.unconditional_channel_context[None].repeat(n, 1))
    return eu + (ec - eu) * float(cfg_scale)


def cpu_loop(od, oc, cfg_scale, lv, table, latent, noise, prediction="epsilon", reference=None, mask=None, refiner=False, draw0=0):
    """One trajectory piece in fp32 torch on the CPU around the oracle's UNet, advanced with the fp64 rows of `table` on the schedule lv from
    `latent`.  noise(draw) -> the tensor of that draw number (the tests fetch it from the GPU generator); the piece counts its iterations
    from 0 as a call of the engine does.  The histories start empty: a table whose order restarts goes with a piece that starts one."""
    assert len(lv) == len(table)
    draw_blend, draw_sigma = (lambda i: 1 + 2 * i), (lambda i: 2 + 2 * i)
    x0p, x0pp = torch.zeros_like(latent), torch.zeros_like(latent)
    for i, (t, a, ap) in enumerate(lv):
        if mask is not None:
            latent = torch.where(mask, latent, reference * (a ** 0.5) + noise(draw_blend(i)) * ((1.0 - a) ** 0.5))
        out = unet_eps(od, oc, latent, t, cfg_scale, refiner)
        x0 = latent * (a ** 0.5) - out * ((1.0 - a) ** 0.5) if prediction == "v" else (latent - out * ((1.0 - a) ** 0.5)) / (a ** 0.5)
        c_x, c_0, c_1, c_2, c_z = (float(v) for v in table[i])
        latent = latent * c_x + x0 * c_0 + x0p * c_1 + x0pp * c_2
        if c_z != 0.0:
            latent = latent + noise(draw_sigma(i)) * c_z
        x0pp, x0p = x0p, x0
    return latent
