"""Guidance options, host side (no GPU): sdxl_guidance_default / sdxl_guidance_check with every refusal and its message, the struct layout
of the binding, and the properties of the fp64 reference (tests/guidance_ref.py) the GPU tests compare against."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import guidance_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sdxl_guidance_default", "sdxl_guidance_check", "sdxl_diffuser_set_guidance", "sdxl_diffuser_get_guidance",
           "sdxl_cfg_rescale_factors")
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def built(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg


def test_header_declares_and_library_exports_the_guidance_symbols(built):
    hdr = open(os.path.join(ROOT, "include", "sdxl_mi355.h")).read()
    declared = set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", hdr))
    l = ctypes.CDLL(built.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and s in built.ABI_SYMBOLS and hasattr(l, s), s
    assert re.search(r"\}\s*sdxl_guidance\s*;", hdr) and "SDXL_GUIDANCE_CFG = 0, SDXL_GUIDANCE_OFF = 1" in hdr
    G = built.Guidance      # { int32 mode; float rescale; int32 n_scales; float scales[8]; int32 t_lo, t_hi; }
    assert ctypes.sizeof(G) == 52
    assert [getattr(G, f).offset for f in ("mode", "rescale", "n_scales", "scales", "t_lo", "t_hi")] == [0, 4, 8, 12, 44, 48]
    assert (built.GUIDANCE_CFG, built.GUIDANCE_OFF) == (0, 1)


def test_default(built):
    g = built.Guidance(7, 0.5, 3, (ctypes.c_float * 8)(*[1.0] * 8), 5, 6)
    built.lib().sdxl_guidance_default(ctypes.byref(g))
    assert (g.mode, g.rescale, g.n_scales, g.t_lo, g.t_hi) == (0, 0.0, 0, 0, INT32_MAX)
    assert list(g.scales) == [0.0] * 8
    assert g == built.guidance_default() == built.make_guidance()
    built.guidance_check(g)
    built.guidance_check(g, is_refiner=True)
    built.lib().sdxl_guidance_default(None)      # tolerated


ACCEPTED = [
    dict(),
    dict(rescale=0.7),
    dict(rescale=1.0),
    dict(scales=[2.0, 7.5]),
    dict(scales=[-1.0]),                          # a negative scale is finite: allowed
    dict(scales=[1.0] * 8),
    dict(t_range=(0, 0)),
    dict(t_range=(250, 750)),
    dict(t_range=(999, INT32_MAX)),
    dict(rescale=0.7, scales=[2.0, 7.5], t_range=(250, 750)),
    dict(mode="off"),
    dict(mode=1),
]

REFUSED = [
    (dict(mode=2), "mode"),
    (dict(mode=-1), "mode"),
    (dict(rescale=-0.1), "rescale"),
    (dict(rescale=1.5), "rescale"),
    (dict(rescale=math.nan), "rescale"),
    (dict(rescale=math.inf), "rescale"),
    (dict(scales=[1.0] * 9), "n_scales"),
    (dict(scales=[1.0, math.inf]), "finite"),
    (dict(scales=[math.nan]), "finite"),
    (dict(t_range=(-1, 10)), "t_lo"),
    (dict(t_range=(500, 499)), "t_lo"),
    (dict(mode="off", rescale=0.5), "SDXL_GUIDANCE_OFF"),
    (dict(mode="off", scales=[1.0]), "SDXL_GUIDANCE_OFF"),
    (dict(mode="off", t_range=(0, 500)), "SDXL_GUIDANCE_OFF"),
    (dict(mode="off", t_range=(1, INT32_MAX)), "SDXL_GUIDANCE_OFF"),
]


@pytest.mark.parametrize("options", ACCEPTED)
def test_check_accepts(built, options):
    g = built.make_guidance(**options)
    assert built.lib().sdxl_guidance_check(ctypes.byref(g), 0) == 0
    built.guidance_check(g)


@pytest.mark.parametrize("options,word", REFUSED)
def test_check_refuses_with_its_message(built, options, word):
    g = built.make_guidance(**options)
    l = built.lib()
    assert l.sdxl_guidance_check(ctypes.byref(g), 0) == 1           # SDXL_ERR_INVALID
    msg = l.sdxl_last_error().decode()
    assert msg.startswith("guidance:") and word in msg, msg
    with pytest.raises(built.InvalidArgument, match=word):
        built.guidance_check(g)


def test_negative_n_scales_and_null(built):
    g = built.guidance_default()
    g.n_scales = -1
    l = built.lib()
    assert l.sdxl_guidance_check(ctypes.byref(g), 0) == 1 and "n_scales" in l.sdxl_last_error().decode()
    assert l.sdxl_guidance_check(None, 0) == 1 and "null" in l.sdxl_last_error().decode()


@pytest.mark.parametrize("options", [dict(rescale=0.7), dict(scales=[2.0]), dict(t_range=(250, 750)), dict(t_range=(0, INT32_MAX - 1))])
def test_refiner_takes_the_default_or_off_only(built, options):
    g = built.make_guidance(**options)
    built.guidance_check(g)
    with pytest.raises(built.InvalidArgument, match="refiner"):
        built.guidance_check(g, is_refiner=True)
    built.guidance_check(built.make_guidance(mode="off"), is_refiner=True)
    built.guidance_check(built.guidance_default(), is_refiner=True)


def test_first_complaint_wins(built):
    """the order of the header's list: mode, rescale, n_scales, scales, interval, OFF's companions, refiner"""
    g = built.make_guidance(mode=5, rescale=2.0, scales=[math.nan], t_range=(3, 2))
    order = [("mode", lambda: setattr(g, "mode", 0)), ("rescale", lambda: setattr(g, "rescale", 0.5)),
             ("finite", lambda: g.scales.__setitem__(0, 1.0)), ("t_lo", lambda: setattr(g, "t_hi", 9))]
    for word, fix in order:
        with pytest.raises(built.InvalidArgument, match=word):
            built.guidance_check(g, is_refiner=True)
        fix()
    with pytest.raises(built.InvalidArgument, match="refiner"):
        built.guidance_check(g, is_refiner=True)
    built.guidance_check(g)


# ------------------------------------------------------------------------------------------------ the reference itself

def _pair(n=3, m=200, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, m, 4)), rng.standard_normal((n, m, 4))


def test_reference_phi_0_is_1_and_phi_1_is_the_ratio():
    ec, eu = _pair()
    s = [7.5, 2.0, -1.5]
    assert np.array_equal(GR.rescale_factors(ec, eu, s, 0.0), np.ones(3))
    r = GR.rescale_factors(ec, eu, s, 1.0)
    for b in range(3):
        ecfg = eu[b] + (ec[b] - eu[b]) * s[b]
        assert r[b] == pytest.approx(ec[b].std() / ecfg.std(), rel=1e-14)
        assert r[b] == pytest.approx(ec[b].std(ddof=1) / ecfg.std(ddof=1), rel=1e-14)      # N or N - 1: the same ratio
    half = GR.rescale_factors(ec, eu, s, 0.5)
    assert np.allclose(half, 0.5 * r + 0.5, rtol=1e-15)
    assert np.all(r[:2] < 1.0)                     # guidance widens the spread on independent branches


def test_reference_scale_1_gives_1_and_constant_gives_1():
    ec, eu = _pair()
    assert np.allclose(GR.rescale_factors(ec, eu, [1.0] * 3, 0.7), 1.0, rtol=1e-14)       # ecfg == ec
    c = np.full((2, 50, 4), 0.25)
    assert np.array_equal(GR.rescale_factors(c, c, [7.5, 2.0], 0.7), np.ones(2))          # M2(ecfg) == 0
    assert np.array_equal(GR.rescale_factors_f32(c, c, [7.5, 2.0], 0.7), np.ones(2, np.float32))


def test_reference_is_shift_invariant_and_the_f32_form_is_close():
    ec, eu = _pair(seed=6)
    s = [7.5, 2.0, 4.0]
    f = GR.rescale_factors(ec, eu, s, 0.7)
    assert np.allclose(GR.rescale_factors(ec + 100.0, eu + 100.0, s, 0.7), f, rtol=1e-12)
    ec32, eu32 = ec.astype(np.float32), eu.astype(np.float32)
    err = np.abs(GR.rescale_factors_f32(ec32, eu32, s, 0.7) - GR.rescale_factors(ec32, eu32, s, 0.7)) / f
    assert err.max() < 1e-6


def test_active_range_is_the_middle_half():
    from oracle import config as OC
    import solver_ref as R
    alphas = OC.alphas_cumprod()
    for n_steps, want in ((4, 2), (8, 4)):
        lo, hi = GR.active_range(alphas, n_steps)
        ts = [t for t, _, _ in R.schedule(alphas, n_steps)]
        on = [lo <= t <= hi for t in ts]
        assert sum(on) == want and not on[0] and not on[-1]
