"""sdxl_solver_coefficients (host logic, no device): the table the sampler uploads, against the fp64 restatement of
tests/solver_ref.py, on oracle.config.alphas_cumprod().  The function is the one Diffuser::diffuse fills its DPM-Solver++(2M)
table from, so these tests check what the GPU runs."""
import ctypes
import math
import os

import numpy as np
import pytest

import solver_ref as R
from oracle import config as OC

ALPHAS = OC.alphas_cumprod()
SHAPES = [(4, 0), (5, 0), (8, 0), (30, 0), (50, 0), (100, 0), (50, 800)]      # (n_steps, step_start); the last is the refiner's
ETAS = [0.0, 0.5, 1.0]
REL = 1e-12                  # both sides are f64 evaluations of the same short expressions: a few hundred ulp, far below the 6e-8
                             # at which the fp32 table entry would change


@pytest.fixture(scope="module")
def built(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg


def close(got, want):
    return np.abs(got - want) <= REL * np.abs(want)


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("n_steps,step_start", SHAPES)
@pytest.mark.parametrize("solver", [R.DDIM, R.DPMPP_2M])
def test_coefficients_against_restatement(built, solver, n_steps, step_start, eta):
    got = built.solver_coefficients(ALPHAS, n_steps, step_start, solver=solver, eta=eta)
    want = R.coefficients(ALPHAS, n_steps, step_start, solver=solver, eta=eta)
    assert got.dtype == np.float64 and got.shape == (built.step_count(n_steps, step_start, len(ALPHAS)), 4)
    assert got.shape == want.shape
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print(f"solver={solver} n_steps={n_steps} step_start={step_start} eta={eta}: worst relative difference {rel[want != 0].max():.2e}")
    assert close(got, want).all(), (got - want)


@pytest.mark.parametrize("n_steps,step_start", SHAPES)
def test_table_structure(built, n_steps, step_start):
    for eta in ETAS:
        t = built.solver_coefficients(ALPHAS, n_steps, step_start, solver=built.SOLVER_DPMPP_2M, eta=eta)
        assert t[0, 2] == 0.0, "iteration 0 has no history"
        assert (t[1:-1, 2] < 0.0).all(), "every inner iteration is second order"
        assert tuple(t[-1]) == (0.0, 1.0, 0.0, 0.0), "ap == 1: the last iteration returns x0"
        assert np.isfinite(t).all()
        if eta == 0.0:
            assert (t[:, 3] == 0.0).all()
        else:
            assert (t[:-1, 3] > 0.0).all()
    # first-order 2M rows at eta = 0 are DDIM's
    ddim = built.solver_coefficients(ALPHAS, n_steps, step_start, solver=built.SOLVER_DDIM, eta=0.0)
    two_m = built.solver_coefficients(ALPHAS, n_steps, step_start, solver=built.SOLVER_DPMPP_2M, eta=0.0)
    for i in (0, len(ddim) - 1):
        assert np.abs(two_m[i] - ddim[i]).max() <= REL, (i, two_m[i], ddim[i])


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("n_steps,step_start", SHAPES)
def test_ddim_rows_restate_diffuse(built, n_steps, step_start, eta):
    """sqrt_ap, sqrt_1map, sigma as Diffuser::diffuse computes them, folded into (c_x, c_0, 0, sigma)"""
    t = built.solver_coefficients(ALPHAS, n_steps, step_start, solver=built.SOLVER_DDIM, eta=eta)
    for i, (_, a, ap) in enumerate(R.schedule(ALPHAS, n_steps, step_start)):
        sigma = 0.0 if eta == 0.0 else eta * math.sqrt((1.0 - ap) / (1.0 - a)) * math.sqrt(1.0 - a / ap)
        sqrt_ap, sqrt_1map = math.sqrt(ap), math.sqrt(max(1.0 - ap - sigma * sigma, 0.0))
        want = np.array([sqrt_1map / math.sqrt(1.0 - a), sqrt_ap - sqrt_1map * math.sqrt(a) / math.sqrt(1.0 - a), 0.0, sigma])
        assert np.abs(t[i] - want).max() <= REL, (i, t[i], want)


@pytest.mark.parametrize("n_steps", [10, 20, 40, 50, 100])
def test_second_order_accuracy_on_gaussian_data(built, n_steps):
    """The restatement alone gives DDIM / 2M error ratios of 6.9 - 14.8 on these step counts, so one third is a condition with a
    factor-two margin; a sign error in c_1 or a wrong r makes 2M worse than DDIM."""
    ddim = R.analytic_errors(ALPHAS, n_steps, built.solver_coefficients(ALPHAS, n_steps, solver=built.SOLVER_DDIM))
    two_m = R.analytic_errors(ALPHAS, n_steps, built.solver_coefficients(ALPHAS, n_steps, solver=built.SOLVER_DPMPP_2M))
    print(f"n_steps={n_steps}: relative error DDIM {ddim:.3e}, 2M {two_m:.3e}, ratio {ddim / two_m:.2f}")
    assert two_m <= ddim / 3.0


def test_argument_errors(built):
    l = built.lib()
    a = np.ascontiguousarray(ALPHAS, dtype=np.float32)
    pa = a.ctypes.data_as(ctypes.c_void_p)
    out = np.full(4 * 64, 7.25, dtype=np.float64)
    po = out.ctypes.data_as(ctypes.c_void_p)

    def call(alphas=pa, n_train=1000, n_steps=4, step_start=0, solver=1, eta=0.0, o=po, cap=64):
        return l.sdxl_solver_coefficients(alphas, n_train, n_steps, step_start, solver, ctypes.c_double(eta), o, cap)

    bad = [dict(eta=-0.1), dict(eta=1.5), dict(eta=float("nan")), dict(eta=float("inf")), dict(n_steps=0), dict(n_steps=1001),
           dict(n_steps=-3), dict(cap=3), dict(cap=0), dict(solver=7), dict(solver=-1), dict(step_start=-1), dict(step_start=1000),
           dict(alphas=None), dict(o=None), dict(n_train=0)]
    for kw in bad:
        assert call(**kw) == 1, kw                                         # SDXL_ERR_INVALID
        assert l.sdxl_last_error().decode(), kw
        assert (out == 7.25).all(), f"{kw}: out was written"
    assert call(solver=7) == 1 and "solver" in l.sdxl_last_error().decode()
    assert call(eta=2.0) == 1 and "eta" in l.sdxl_last_error().decode()
    assert call(cap=4) == 0 and (out[:16] != 7.25).all() and (out[16:] == 7.25).all()
    for kw in (dict(solver="euler"), dict(eta=1.5), dict(n_steps=0)):
        with pytest.raises(built.EngineError):
            built.solver_coefficients(ALPHAS, **{"n_steps": 4, **kw})


def test_python_names(built):
    assert (built.SOLVER_DDIM, built.SOLVER_DPMPP_2M) == (0, 1)
    by_name = built.solver_coefficients(ALPHAS, 8, solver="dpmpp_2m", eta=0.5)
    assert np.array_equal(by_name, built.solver_coefficients(ALPHAS, 8, solver=built.SOLVER_DPMPP_2M, eta=0.5))
    assert np.array_equal(built.solver_coefficients(ALPHAS, 8, solver="ddim"), built.solver_coefficients(ALPHAS, 8, solver=0))
