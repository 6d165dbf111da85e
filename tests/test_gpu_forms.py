"""The transformer projection forms of the split-operand UNet (csrc/unet.cpp plan_transformer, csrc/engine.h LinForm) against fp64, op by op.

Every case runs ONE LayerNorm-fed projection through sdxl_transformer_projection, which calls the code UNet::spatial_transformer runs
(WeightBuilder::pack, alloc_ln_operands, want_ln_shadow, ln_input): a producer (out-projection / FF-out, form NATIVE, F16 or X2) adds into the
fp32 stream t, then LayerNorm(t) feeds the consumer in its form -- through the LayerNorm launch ("ln") or through the shadow the producer
left ("sh", MIX_LN_SHADOW).  The consumer is checked against the engine's own fp32 t (returned by the entry), so a bar measures the
consumer alone; the producer is checked against fp64 on its own.

Bars (derivations):
  * fp32-class forms (NATIVE, X2, F16_AHILO; both paths) and the producers: max |out - ref| <= 5e-6 max |ref| against fp64
    LN(t) W + b (+ GEGLU in fp64) -- the bar of test_linear_split_operand.  The operands carry ~22 significant bits ((hi, lo) f16 pairs,
    or f16 weights times (hi, lo) activations), the accumulation is fp32: ~1e-7 measured, 5e-6 leaves room for K = 5120.
  * activation-rounding forms (F16, F16_WHILO, the f16 shadow): compared with an fp64 EMULATION of exactly the roundings the form claims:
      LayerNorm launch:  f16(LN(t)) W + b                          (W = the f16 weights for F16, the unrounded fp32 weights for WHILO)
      f16 shadow:        rstd (f16(t o gamma) W) - rstd mu (gamma W) + beta W + b
    The kernel rounds an fp32 value to f16; the emulation rounds the exact one.  Where the exact value lies within the fp32 round-off of
    that value (2^-21 relative for the LayerNorm, 2^-23 for the product t gamma) of an f16 rounding midpoint, the two may round to
    neighbouring f16 numbers: each such element may move its products by one f16 spacing, so the bar of output (m, n) gets
    sum_k spacing(m, k) |W(k, n)| (x rstd for the shadow; through the GEGLU with |gelu'| <= 1.13) on top of 5e-6 max |ref|.
    A lost weight lo half (WHILO) or any other extra rounding adds ~2^-12 sqrt(K) |a| |w| to EVERY output: far outside that bar.
  * outputs stored as f16 (an f16 QKV projection writes f16 for the f16 self-attention; GEGLU outputs at M < 256 are f16, widened):
    + half an f16 spacing at the reference value.
"""
import math

import pytest
import torch

from util import f16v, geglu, rounding_slack, seeded, ulp16

pytestmark = pytest.mark.gpu

U32 = 5e-6           # fp32-class bar (test_linear_split_operand)
EPS = 1e-5
NATIVE, F16, WHILO, AHILO, X2 = 0, 1, 2, 3, 4
QKV, QUERY, GEGLU = 0, 1, 2
FORM_NAME = {NATIVE: "NATIVE", F16: "F16", WHILO: "F16_WHILO", AHILO: "F16_AHILO", X2: "X2"}


class Case:
    """seeded inputs of one projection: r [M, C], producer a [M, Kp] @ wp [Kp, C] + bp, LayerNorm (gamma, beta), consumer w [C, N] + b"""

    def __init__(self, C, rows, B, N, Kp, seed=0, f16_weights=True):
        M = rows * B
        self.C, self.rows, self.B, self.N, self.Kp, self.M = C, rows, B, N, Kp, M
        self.r = seeded(M, C, seed=seed)
        self.a = seeded(M, Kp, seed=seed + 1)
        self.wp = f16v(seeded(Kp, C, seed=seed + 2) * (0.5 / math.sqrt(Kp)))
        self.bp = 0.1 * seeded(C, seed=seed + 3)
        self.gamma, self.beta = 1 + 0.1 * seeded(C, seed=seed + 4), 0.1 * seeded(C, seed=seed + 5)
        self.w = seeded(C, N, seed=seed + 6) / math.sqrt(C)
        if f16_weights:
            self.w = f16v(self.w)
        self.b = 0.1 * seeded(N, seed=seed + 7)

    def run(self, pkg, ctx, proj, form, shadow, pform, entries=None):
        """-> (out, t, shadow_taken); entries = (first, count): only those batch entries"""
        sl = slice(None)
        B = self.B
        if entries is not None:
            sl = slice(entries[0] * self.rows, (entries[0] + entries[1]) * self.rows)
            B = entries[1]
        producer = None if pform is None else (self.a[sl].cuda(), self.wp.cuda(), self.bp.cuda(), pform)
        return pkg.transformer_projection(ctx, self.r[sl].cuda(), self.gamma.cuda(), self.beta.cuda(), self.w.cuda(), self.b.cuda(), proj, form,
                                          EPS, shadow, producer, batch=B)

    def stream_ref(self, pform):
        """fp64 t = r + a wp + bp (an f16 producer reads f16(a); NATIVE / X2 read its HL16 rows: ~22 bits)"""
        a = (f16v(self.a) if pform == F16 else self.a).double().cuda()
        return self.r.double().cuda() + a @ self.wp.double().cuda() + self.bp.double().cuda()


def reference(case, t, proj, form, from_shadow, out16):
    """(reference, per-element bar) for the consumer's output on the engine's stream t (see the module docstring)"""
    W, b = case.w.double().cuda(), case.b.double().cuda()
    gamma, beta = case.gamma.double().cuda(), case.beta.double().cuda()
    td = t.double()
    mu = td.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((td - mu) ** 2).mean(-1, keepdim=True) + EPS)
    x = (td - mu) * rstd * gamma + beta
    g = proj == GEGLU
    if form in (NATIVE, X2, AHILO):
        y = x @ W + b
        ref, slack = geglu(y) if g else (y, None)
    elif from_shadow:
        s = td * gamma
        h, sp = rounding_slack(s, 2.0 ** -23 * s.abs())
        y = rstd * (h @ W) - rstd * mu * (gamma @ W) + beta @ W + b
        dy = rstd * (sp @ W.abs())
        ref, slack = geglu(y, dy) if g else (y, dy)
    else:
        h, sp = rounding_slack(x, 2.0 ** -21 * (x.abs() + rstd * (td * gamma).abs() + beta.abs()))
        Wf = W if form == WHILO else W.float().half().double()
        y = h @ Wf + b
        dy = sp @ Wf.abs()
        ref, slack = geglu(y, dy) if g else (y, dy)
    tol = U32 * ref.abs().max() + (slack if slack is not None else 0.0)
    if out16:
        tol = tol + ulp16(ref.abs() + tol) / 2
    return ref, tol


def out_is_f16(case, proj, form, took):
    """the consumer's stored output is f16: an f16 QKV projection (for the f16 self-attention); a GEGLU output at M < 256 that is widened"""
    if proj == QKV:
        return form == F16
    return proj == GEGLU and case.M < 256 and (took or form in (F16, WHILO, AHILO))


def check(case, out, t, proj, form, took, label):
    ref, tol = reference(case, t, proj, form, took, out_is_f16(case, proj, form, took))
    err = (out.double() - ref).abs()
    assert torch.isfinite(out).all(), label
    worst = float((err / tol).max())
    rel = float(err.max() / ref.abs().max())
    print(f"  {label}: max |out - ref| / max |ref| = {rel:.3e}, worst element {worst:.3f} x its bar")
    assert worst <= 1.0, (label, worst, rel)
    return rel


def n_of(proj, C):
    return {QKV: 3 * C, QUERY: C, GEGLU: 8 * C}[proj]


CASES = [  # projection, form, producer form, producer K / C, C, rows per entry, B, paths, shadow taken where asked
    # SDXL's sizes: 64^2 level (C = 640, 4096 rows per entry), 32^2 level (C = 1280, 1024 rows), CFG pair B = 2
    (QKV, NATIVE, NATIVE, 4, 640, 4096, 1, "ln", None),
    (GEGLU, NATIVE, NATIVE, 1, 1280, 1024, 2, "ln", None),
    (QKV, F16, F16, 4, 1280, 1024, 2, "ln sh", True),
    (QUERY, F16, F16, 1, 640, 4096, 1, "ln sh", True),
    (GEGLU, F16, F16, 1, 640, 4096, 1, "ln sh", True),
    (GEGLU, AHILO, F16, 1, 1280, 1024, 2, "ln sh", True),
    (QKV, X2, X2, 4, 640, 4096, 1, "sh", True),        # (the X2 QKV projection exists only as a shadow pair: its plain twin runs where no shadow is taken)
    (QUERY, X2, X2, 1, 1280, 1024, 2, "ln sh", True),
    (GEGLU, X2, X2, 1, 640, 4096, 1, "ln sh", True),   # N = 5120: N % 640 == 0
    # ragged row counts (not multiples of the 256 / 128-row tiles)
    (QUERY, F16, F16, 1, 640, 1000, 2, "ln sh", True),
    (GEGLU, X2, X2, 1, 640, 1000, 1, "sh", True),
    # M < 256: the GEGLU output is f16 and widened (gg_direct off), other tiles
    (GEGLU, F16, F16, 1, 640, 200, 1, "ln sh", True),
    (GEGLU, AHILO, F16, 1, 640, 200, 1, "ln sh", True),
    (GEGLU, X2, X2, 1, 640, 200, 1, "sh", True),
]


def _case_id(c):
    proj, form, pform, kr, C, rows, B, paths, _ = c
    return f"{['qkv', 'q2', 'geglu'][proj]}-{FORM_NAME[form]}-C{C}-{rows}x{B}-{paths.replace(' ', '+')}"


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_projection_form_against_fp64(pkg, ctx, case):
    proj, form, pform, kr, C, rows, B, paths, expect_taken = case
    d = Case(C, rows, B, n_of(proj, C), kr * C, seed=10 * proj + form)
    print(f"{_case_id(case)} (producer {FORM_NAME[pform]}, K = {kr * C}):")
    outs = {}
    for path in paths.split():
        out, t, took = d.run(pkg, ctx, proj, form, path == "sh", pform)
        if path == "sh":
            assert took == expect_taken, f"shadow taken: {took}, expected {expect_taken}"
        else:
            assert not took
        # the producer (out-projection / FF-out) on its own: fp32 class in every form here (f16 weights, an f16 producer's operand is f16(a))
        tref = d.stream_ref(pform)
        te = float((t.double() - tref).abs().max() / tref.abs().max())
        assert te < U32, ("producer", te)
        outs[path] = (out, check(d, out, t, proj, form, took, f"{path}{' (shadow taken)' if took else ''}, producer rel err {te:.2e}"))
    if len(outs) == 2 and form in (F16, AHILO, X2):
        # the shadow twin stays in the class of its LayerNorm-launch twin
        (o_ln, e_ln), (o_sh, e_sh) = outs["ln"], outs["sh"]
        print(f"  shadow / LayerNorm launch error vs its reference: {e_sh / max(e_ln, 1e-30):.2f}")


def test_x2_is_native_in_another_summation_order(pkg, ctx):
    # X2 multiplies the same (hi, lo) activation halves by the same f16 weights as NATIVE (the weight's lo half is zero), in another order
    for proj, C, rows, B in ((QUERY, 1280, 1024, 2), (QKV, 640, 4096, 1)):
        d = Case(C, rows, B, n_of(proj, C), C, seed=3)
        o_n, t_n, _ = d.run(pkg, ctx, proj, NATIVE, False, X2)
        o_x, t_x, took = d.run(pkg, ctx, proj, X2, True, X2)
        assert took and torch.equal(t_n, t_x)
        r = float((o_x - o_n).abs().max() / o_n.abs().max())
        print(f"{['qkv', 'q2'][proj]} C={C}: |X2 (shadow) - NATIVE| / max |NATIVE| = {r:.3e}")
        assert r < U32
        if proj == QUERY:
            o_xl, _, _ = d.run(pkg, ctx, proj, X2, False, X2)
            r2 = float((o_xl - o_n).abs().max() / o_n.abs().max())
            print(f"   X2 (LayerNorm launch) - NATIVE: {r2:.3e}")
            assert r2 < U32


def test_whilo_leaves_the_weights_unrounded(pkg, ctx):
    # SDXL_DTYPE_F32_SPLIT_MIX's GEGLU on fp32 weights (on purpose: not f16 values): WHILO multiplies f16(LN(t)) by the UNROUNDED weights
    # ((hi | lo 2^8) halves against [a | a 2^-8]); plain F16 also rounds the weights.  Against the emulation f16(LN(t)) W (fp64, W unrounded) WHILO
    # is within the per-element bar; what is left of its error is the one-spacing flips of activations the kernel's fp32 LayerNorm rounds the other
    # way (~0.3 per row at C = 640), so its RMS error is small, while the weight rounding moves EVERY output of F16 by ~2^-12 sqrt(K / 3) |a| |w|.
    # Against unrounded fp64 LN(t) W both carry the activation rounding and F16 also the weight rounding: sqrt(2) x the RMS error.
    d = Case(640, 4096, 1, 8 * 640, 640, seed=7, f16_weights=False)
    o_w, t_w, _ = d.run(pkg, ctx, GEGLU, WHILO, False, NATIVE)
    o_f, t_f, _ = d.run(pkg, ctx, GEGLU, F16, False, NATIVE)
    assert torch.equal(t_w, t_f)
    e_w = check(d, o_w, t_w, GEGLU, WHILO, False, "WHILO vs f16(LN) W")
    ref, _ = reference(d, t_w, GEGLU, WHILO, False, False)
    r64, _ = reference(d, t_w, GEGLU, NATIVE, False, False)
    rms = lambda o, r: float(((o.double() - r) ** 2).mean().sqrt() / (r ** 2).mean().sqrt())
    e_f = float((o_f.double() - ref).abs().max() / ref.abs().max())
    q_w, q_f, u_w, u_f = rms(o_w, ref), rms(o_f, ref), rms(o_w, r64), rms(o_f, r64)
    print(f"vs f16(LN) W: max WHILO {e_w:.3e}, F16 {e_f:.3e} ({e_f / e_w:.1f}x); RMS WHILO {q_w:.3e}, F16 {q_f:.3e} ({q_f / q_w:.1f}x)")
    print(f"vs fp64 LN W: RMS WHILO {u_w:.3e}, F16 {u_f:.3e} ({u_f / u_w:.2f}x)")
    assert e_f > 3 * e_w and q_f > 10 * q_w
    assert u_f > 1.25 * u_w


def test_ahilo_is_fp32_class_where_f16_rounds(pkg, ctx):
    # SDXL_DTYPE_F32_SPLIT_MIX_F16W_GEGLU2's GEGLU on f16-valued weights: (hi | lo 2^8) activation halves -> fp32 class; plain F16 rounds the
    # activations (2^-12 relative each).  Both paths; the f16 shadow must stay in its LayerNorm launch's class.
    d = Case(1280, 1024, 2, 8 * 1280, 1280, seed=11)
    e = {}
    for form in (AHILO, F16):
        for sh in (False, True):
            out, t, took = d.run(pkg, ctx, GEGLU, form, sh, F16)
            assert took == sh
            ref, _ = reference(d, t, GEGLU, NATIVE, False, False)
            e[form, sh] = float((out.double() - ref).abs().max() / ref.abs().max())
    print("vs fp64 LN(t) W: " + ", ".join(f"{FORM_NAME[f]} {'shadow' if s else 'launch'} {v:.3e}" for (f, s), v in e.items()))
    for sh in (False, True):
        assert e[AHILO, sh] < U32
        assert 10 * e[AHILO, sh] < e[F16, sh]
    assert e[F16, True] < 2 * e[F16, False]


def test_f16_shadow_error_scales_with_the_row_mean(pkg, ctx):
    # The f16 shadow rounds t o gamma BEFORE centring: its rounding error is 2^-12 |t| |gamma| per element, normalised by rstd afterwards, so
    # relative to the LayerNorm launch (which rounds the centred (t - mu) rstd gamma + beta) a row's error grows by s = sqrt(mu^2 + sigma^2) rstd
    # (= sqrt(mu^2 + sigma^2) / sigma where sigma^2 >> eps).  Rows with mu / sigma = 0, 4, 16, 800 and a zero-variance row (s = |t| / sqrt(eps)).
    # Asserted: every row of the shadow within 4 s e0 and every row of the launch within 4 e0, e0 = the launch's median row error at mu = 0.
    C, rows = 640, 4096
    d = Case(C, rows, 1, C, C, seed=5)
    z = seeded(rows, C, seed=40)
    g = torch.arange(rows) % 5
    r = z.clone()
    r[g == 1] += 4.0
    r[g == 2] += 16.0
    r[g == 3] = 40.0 + 0.05 * z[g == 3]
    r[g == 4] = 7.0
    d.r = r
    d.a = torch.zeros_like(d.a)           # t = r exactly: the rows' statistics are the designed ones
    d.bp = torch.zeros_like(d.bp)
    res = {}
    for sh in (False, True):
        out, t, took = d.run(pkg, ctx, QUERY, F16, sh, F16)
        assert took == sh and torch.equal(t.cpu(), r)
        assert torch.isfinite(out).all()
        ref, _ = reference(d, t, QUERY, NATIVE, False, False)
        res[sh] = (out.double() - ref).abs().max(-1).values.cpu()
    td = r.double()
    mu, var = td.mean(-1), td.var(-1, unbiased=False)
    s = torch.sqrt(mu ** 2 + var) / torch.sqrt(var + EPS)
    e0 = float(res[False][g == 0].median())
    names = ["mu/sigma 0", "mu/sigma 4", "mu/sigma 16", "mu/sigma 800", "zero variance"]
    for k in range(5):
        m = g == k
        print(f"{names[k]:>14}: s = {float(s[m].median()):9.1f}; row error / e0: launch {float((res[False][m] / e0).median()):6.2f} (max "
              f"{float((res[False][m] / e0).max()):6.2f}), shadow {float((res[True][m] / e0).median()):9.2f}; shadow / (s e0) median "
              f"{float((res[True][m] / (s[m] * e0)).median()):.2f} max {float((res[True][m] / (s[m] * e0)).max()):.2f}")
    print(f"e0 = {e0:.3e} (max |ref| {float(ref.abs().max()):.2f})")
    assert (res[False] <= 4 * e0).all()
    assert (res[True] <= 4 * s * e0).all()


@pytest.mark.parametrize("proj,form,C,rows,kr", [(QUERY, F16, 1280, 1024, 1), (QKV, X2, 640, 1024, 4), (GEGLU, AHILO, 1280, 1024, 1)])
def test_batch_entries_are_independent(pkg, ctx, proj, form, C, rows, kr):
    # entry 1 of a B = 2 run is bit for bit that entry run alone: the kernel selection looks at one entry's rows (rpb), the shadow and the
    # row statistics are per row
    pform = X2 if form == X2 else F16
    d = Case(C, rows, 2, n_of(proj, C), kr * C, seed=21)
    o2, t2, took2 = d.run(pkg, ctx, proj, form, True, pform)
    o1, t1, took1 = d.run(pkg, ctx, proj, form, True, pform, entries=(1, 1))
    print(f"{['qkv', 'q2', 'geglu'][proj]} {FORM_NAME[form]}: shadow taken B=2 {took2}, alone {took1}")
    assert took1 == took2
    assert torch.equal(t2[rows:], t1) and torch.equal(o2[rows:], o1)


def test_refused_shadow_falls_back_bit_for_bit(pkg, ctx):
    # a producer shape the weights-in-registers kernel is not selected for (4096 rows x N = 768, a refiner-like width): no shadow is written,
    # the consumer runs the LayerNorm launch + its plain twin -- bit-identical to the run that never asked for a shadow
    C = 768
    d = Case(C, 4096, 1, 8 * C, C, seed=31)
    o_s, t_s, took = d.run(pkg, ctx, GEGLU, F16, True, F16)
    o_l, t_l, took_l = d.run(pkg, ctx, GEGLU, F16, False, F16)
    print(f"C={C} 4096 rows: shadow taken {took}")
    assert not took and not took_l
    assert torch.equal(t_s, t_l) and torch.equal(o_s, o_l)
    check(d, o_s, t_s, GEGLU, F16, False, "refused shadow")


def test_unsupported_arguments_are_refused(pkg, ctx):
    def call(C, N, proj, form, shadow, pform, Kp=None, f16_weights=True):
        d = Case(C, 64, 1, N, Kp or C, seed=1, f16_weights=f16_weights)
        return d.run(pkg, ctx, proj, form, shadow, pform)

    bad = [
        dict(C=128, N=128, proj=QUERY, form=X2, shadow=False, pform=X2, Kp=48),          # X2 producer, K % 32 != 0
        dict(C=96, N=96 * 3, proj=QKV, form=F16, shadow=True, pform=F16),                # shadow with C % 64 != 0
        dict(C=128, N=1024, proj=GEGLU, form=AHILO, shadow=False, pform=None, f16_weights=False),   # AHILO on weights that are not f16 values
        dict(C=128, N=128, proj=QUERY, form=X2, shadow=False, pform=None, f16_weights=False),       # X2 likewise
        dict(C=128, N=1024, proj=GEGLU, form=X2, shadow=False, pform=None),              # X2 GEGLU with N % 640 != 0
        dict(C=128, N=384, proj=QKV, form=X2, shadow=False, pform=X2),                   # X2 QKV without its shadow pair
        dict(C=128, N=384, proj=QKV, form=WHILO, shadow=False, pform=None),              # (hi | lo) forms are GEGLU forms
        dict(C=128, N=128, proj=QUERY, form=F16, shadow=True, pform=NATIVE),             # a NATIVE producer leaves no shadow
        dict(C=80, N=128, proj=QUERY, form=NATIVE, shadow=False, pform=None),            # C % 32 != 0
    ]
    for kw in bad:
        with pytest.raises(pkg.InvalidArgument):
            call(**kw)
    out, _, _ = call(C=128, N=128, proj=QUERY, form=X2, shadow=False, pform=X2)      # the entry still works afterwards
    assert torch.isfinite(out).all()
