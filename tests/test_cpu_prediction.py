"""Host logic of v-prediction and zero-terminal-SNR schedules (no device): sdxl_rescale_zero_terminal_snr and sdxl_solver_coefficients_pred
against the fp64 restatement of tests/prediction_ref.py."""
import ctypes
import os

import numpy as np
import pytest

import prediction_ref as P
import solver_ref as R

REL = 1e-12                  # the relative tolerance tests/test_cpu_solver.py uses for the 2M table: both sides are f64 evaluations
SOLVERS = [R.DDIM, R.DPMPP_2M]
ETAS = [0.0, 0.5, 1.0]
STEPS = [4, 5, 8, 30]
EPS, V = 0, 1


@pytest.fixture(scope="module")
def built(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg


@pytest.fixture(scope="module")
def zt(built):
    return built.rescale_zero_terminal_snr(built.default_alphas_cumprod())


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------ the rescale helper

def test_rescale_against_restatement(built):
    a = np.ascontiguousarray(built.default_alphas_cumprod(), dtype=np.float32)
    got = built.rescale_zero_terminal_snr(a)
    want64, want = P.rescale_zero_terminal_snr(a)
    assert got.dtype == np.float32 and got.shape == a.shape
    if np.array_equal(got.view(np.int32), want.view(np.int32)):
        print("rescale: bit for bit the fp64 restatement cast to fp32")
    else:
        # the two f64 evaluations may differ by an ulp, which moves an fp32 cast that sits on a rounding boundary: one fp32 ulp allowed
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        print(f"rescale: {int((ulps != 0).sum())} of {a.size} values differ from the restatement, by at most {int(ulps.max())} fp32 ulp")
        assert ulps.max() <= 1
    assert got[-1] == 0.0 and got[0] == a[0]
    assert (np.diff(got.astype(np.float64)) < 0).all(), "not strictly decreasing"
    assert ((got[:-1] > 0) & (got[:-1] < 1)).all()


def test_rescale_in_place_and_refusals(built):
    l = built.lib()
    a = np.ascontiguousarray(built.default_alphas_cumprod(), dtype=np.float32)
    want = built.rescale_zero_terminal_snr(a)
    buf = a.copy()
    assert l.sdxl_rescale_zero_terminal_snr(_p(buf), len(buf), _p(buf)) == 0
    assert np.array_equal(buf.view(np.int32), want.view(np.int32)), "in == out gives other values"

    def refused(inp, n, give_out=True):
        out = np.full(max(len(a), 4), 7.25, dtype=np.float32)
        rc = l.sdxl_rescale_zero_terminal_snr(None if inp is None else _p(inp), n, _p(out) if give_out else None)
        assert rc == 1 and l.sdxl_last_error().decode()                    # SDXL_ERR_INVALID
        assert (out == 7.25).all(), "out was written"

    refused(a, 1)
    refused(a, 0)
    refused(a, -5)
    refused(None, len(a))
    refused(a, len(a), give_out=False)
    for i, bad in ((0, 1.0), (3, 0.0), (len(a) - 1, 0.0), (10, -0.5), (10, 1.5), (10, float("nan"))):
        b = a.copy()
        b[i] = bad
        refused(b, len(b))
    b = a.copy()
    b[501] = b[500]                      # not strictly decreasing
    refused(b, len(b))
    b[501] = np.nextafter(b[500], np.float32(1))
    refused(b, len(b))
    refused(want, len(want))             # a table that already ends in 0 is outside (0, 1)
    with pytest.raises(built.InvalidArgument):
        built.rescale_zero_terminal_snr(want)


# ------------------------------------------------------------------------------------------------ the coefficient table

@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("n_steps", STEPS)
@pytest.mark.parametrize("solver", SOLVERS)
def test_coefficients_on_the_zero_terminal_table(built, zt, solver, n_steps, eta):
    got = built.solver_coefficients(zt, n_steps, solver=solver, eta=eta, prediction="v")
    want = P.coefficients(zt, n_steps, 0, solver, eta)
    assert got.dtype == np.float64 and got.shape == want.shape == (built.step_count(n_steps, 0, len(zt)), 4)
    assert np.isfinite(got).all()
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print(f"solver={solver} n_steps={n_steps} eta={eta}: worst relative difference {rel[want != 0].max():.2e}")
    assert (np.abs(got - want) <= REL * np.abs(want)).all(), (got - want)
    if solver == R.DPMPP_2M:
        ap = float(np.float64(zt[999 - 1000 // n_steps]))
        row0 = (np.sqrt(1.0 - ap), np.sqrt(ap), 0.0, 0.0) if eta == 0.0 else (0.0, np.sqrt(ap), 0.0, np.sqrt(1.0 - ap))
        assert tuple(got[0]) == row0, "row 0 is the limit at lambda = -inf, exactly"
        assert got[1, 2] == 0.0, "the iteration behind a == 0 is first order"
        assert got[2, 2] != 0.0, "the one after it is second order"
        assert tuple(got[-1]) == (0.0, 1.0, 0.0, 0.0)


def test_orientation_rows(built, zt):
    """The rows at n_steps = 4, eta = 0 as they were written down for orientation, from the rescaled table held in f64.  The entry takes the
    table as fp32 (each alphas_cumprod value moved by up to 2^-24 relative, 6e-8), and a row is a smooth function of three of them with
    derivatives of order 1: 2e-7 is that, not a measurement.  A wrong limit or a wrong order moves a row by 1e-2 and more."""
    got = built.solver_coefficients(zt, 4, solver="dpmpp_2m", eta=0.0, prediction="v")
    want = np.array([(0.98327439, 0.18213040, 0, 0), (0.88523171, 0.33107227, 0, 0), (0.67559700, 0.66578021, -0.18955701, 0), (0, 1, 0, 0)])
    print(f"orientation rows: largest difference {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() < 2e-7, got


@pytest.mark.parametrize("solver", SOLVERS)
def test_pred_entry_agrees_with_the_old_entry(built, solver):
    """on a table without a zero the rows do not depend on the prediction type: the same f64 bits from all three calls"""
    a = built.default_alphas_cumprod()
    for n_steps, step_start in ((4, 0), (8, 0), (30, 0), (50, 800)):
        for eta in ETAS:
            old = built.solver_coefficients(a, n_steps, step_start, solver=solver, eta=eta)
            for pred in (EPS, V):
                new = np.zeros_like(old)
                af = np.ascontiguousarray(a, dtype=np.float32)
                rc = built.lib().sdxl_solver_coefficients_pred(_p(af), len(af), n_steps, step_start, solver, pred, ctypes.c_double(eta), _p(new),
                                                               len(new))
                assert rc == 0
                assert np.array_equal(old.view(np.int64), new.view(np.int64)), (solver, n_steps, step_start, eta, pred)


def test_refusals(built, zt):
    l = built.lib()
    out = np.full(4 * 64, 7.25, dtype=np.float64)

    def call(alphas=zt, n_steps=4, step_start=0, solver=1, pred=V, eta=0.0, cap=64):
        return l.sdxl_solver_coefficients_pred(_p(alphas), len(alphas), n_steps, step_start, solver, pred, ctypes.c_double(eta), _p(out), cap)

    for solver in SOLVERS:
        assert call(solver=solver, pred=EPS) == 1                          # SDXL_ERR_INVALID
        assert "prediction" in l.sdxl_last_error().decode()
        assert (out == 7.25).all()
        # the old entry is the _pred entry with SDXL_PREDICTION_EPSILON
        assert l.sdxl_solver_coefficients(_p(zt), len(zt), 4, 0, solver, ctypes.c_double(0.0), _p(out), 64) == 1
        assert "prediction" in l.sdxl_last_error().decode() and (out == 7.25).all()
    for bad in (2, -1, 7):
        assert call(pred=bad) == 1 and "prediction" in l.sdxl_last_error().decode()
        assert (out == 7.25).all()
    # a == 0 is admitted at an iteration's own timestep only: a zero where a step lands (ap), or a value of 1, stays refused under v
    b = zt.copy()
    b[749] = 0.0
    assert call(alphas=b) == 1 and (out == 7.25).all()
    b = zt.copy()
    b[999] = 1.0
    assert call(alphas=b) == 1 and (out == 7.25).all()
    assert call(eta=1.5) == 1 and call(cap=3) == 1 and call(solver=7) == 1 and (out == 7.25).all()
    # refine_latent's shape on the zero-terminal table does not touch t = T - 1
    assert call(n_steps=50, step_start=800) == 0
    out[:] = 7.25
    assert call() == 0 and (out[:16] != 7.25).any() and (out[16:] == 7.25).all()
    with pytest.raises(built.InvalidArgument, match="prediction"):
        built.solver_coefficients(zt, 4)
    with pytest.raises(built.InvalidArgument, match="prediction"):
        built.solver_coefficients(zt, 4, prediction="sample")


def test_python_names(built, zt):
    assert (built.PREDICTION_EPSILON, built.PREDICTION_V) == (0, 1)
    by_name = built.solver_coefficients(zt, 8, solver="dpmpp_2m", eta=0.5, prediction="v")
    assert np.array_equal(by_name, built.solver_coefficients(zt, 8, solver=built.SOLVER_DPMPP_2M, eta=0.5, prediction=built.PREDICTION_V))
    a = built.default_alphas_cumprod()
    assert np.array_equal(built.solver_coefficients(a, 8, prediction="epsilon"), built.solver_coefficients(a, 8, prediction=0))
    assert np.array_equal(built.solver_coefficients(a, 8, prediction="epsilon"), built.solver_coefficients(a, 8))
