"""Noise-level schedules, host logic (no device): the sigma spacings and sigma_to_t against the fp64 restatement of tests/levels_ref.py, the
five-column rows -- the old solvers' bit for bit against the four-column entries, DPM++ 3M SDE against the restatement, which is itself
checked against the literal k-diffusion loop --, every refusal, and the check that the bound of tests/test_gpu_levels_step.py is a condition
the kernel's arithmetic meets (an fp32 numpy emulation of its lines, on that test's inputs)."""
import ctypes
import os

import numpy as np
import pytest

import fewstep_cases as FC
import fewstep_ref as F
import levels_cases as C
import levels_ref as L
import sampler_step_cases as S
import solver_ref as R
from oracle import config as OC

ALPHAS = OC.alphas_cumprod()
REL = 1e-12                  # tests/test_cpu_solver.py's bar and reasoning: both sides are f64 evaluations of the same short expressions
UNEVEN = [900, 650, 300, 20]


@pytest.fixture(scope="module")
def built(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg


def close(got, want, rel=REL):
    return np.abs(np.asarray(got) - np.asarray(want)) <= rel * np.abs(np.asarray(want))


# ------------------------------------------------------------------------------------------------ spacings and the mapping

@pytest.mark.parametrize("n", [1, 2, 6, 20, 40])
def test_spacings_against_restatement(built, n):
    for kw in (dict(), dict(sigma_min=0.1, sigma_max=10.0), dict(sigma_max=5.0)):
        k = built.sigma_schedule("karras", n, ALPHAS, rho=7.0, **kw)
        e = built.sigma_schedule("exponential", n, ALPHAS, **kw)
        assert len(k) == len(e) == n
        assert close(k, L.sigmas_karras(n, ALPHAS, **kw)).all() and close(e, L.sigmas_exponential(n, ALPHAS, **kw)).all()
        assert all(b < a for a, b in zip(k, k[1:])) and all(b < a for a, b in zip(e, e[1:])) and min(k + e) > 0.0
        hi = kw.get("sigma_max", L.table_ends(ALPHAS)[1])
        assert close(k[0], hi) and close(e[0], hi), "the first entry is sigma_max (n == 1: the only one)"
    assert close(built.sigma_schedule("karras", n, ALPHAS, rho=3.0), L.sigmas_karras(n, ALPHAS, rho=3.0)).all()
    o = built.sigma_schedule("of_timesteps", n, ALPHAS)
    assert len(o) == built.step_count(n, 0, 1000) and close(o, L.sigmas_of_timesteps(n, ALPHAS)).all()


def test_table_ends(built):
    lo, hi = L.table_ends(ALPHAS)
    assert abs(lo - 0.02917) < 1e-5 and abs(hi - 14.6146) < 1e-4
    k = built.sigma_schedule("karras", 6)
    assert close(k[0], hi) and close(k[-1], lo)
    assert built.sigma_schedule(built.SIGMAS_EXPONENTIAL, 4) == built.sigma_schedule("exponential", 4, ALPHAS)


def test_sigma_to_timestep(built):
    lo, hi = L.table_ends(ALPHAS)
    for s in [hi, lo, 1.0, 0.5, 3.3, 14.0, 0.03] + L.sigmas_karras(9, ALPHAS) + L.sigmas_exponential(7, ALPHAS):
        assert abs(built.sigma_to_timestep(s, ALPHAS) - L.sigma_to_t(ALPHAS, s)) <= 1e-9
        assert built.sigma_to_timestep(s, ALPHAS, round_t=True) == L.sigma_to_t(ALPHAS, s, True)
    # outside the table the mapping clamps to its ends
    assert built.sigma_to_timestep(100.0, ALPHAS) == 999.0 and built.sigma_to_timestep(1e-4, ALPHAS) == 0.0
    # the sigmas of the integers come back as the integers: exactly with ROUND_T, to the rounding of two logarithms without
    for n in (4, 30, 1000):
        ts = F.schedule_reference(n)
        assert ts[0] == 999 and (n < 1000 or ts[-1] == 0), "both ends of the table"
        for t, s in zip(ts, built.sigma_schedule("of_timesteps", n, ALPHAS)):
            assert built.sigma_to_timestep(s, ALPHAS, round_t=True) == float(t)
            assert abs(built.sigma_to_timestep(s, ALPHAS) - t) <= 1e-8
    # ties go to even: the sigma half way (in ln sigma) between two training timesteps
    al = np.asarray(ALPHAS, np.float32).astype(np.float64)
    Lj = 0.5 * np.log((1.0 - al) / al)
    for j in (0, 1, 500, 501, 997):
        mid = float(np.exp(0.5 * (Lj[j] + Lj[j + 1])))
        t = built.sigma_to_timestep(mid, ALPHAS)
        assert abs(t - (j + 0.5)) <= 1e-9
        if t == j + 0.5:
            assert built.sigma_to_timestep(mid, ALPHAS, round_t=True) == float(j if j % 2 == 0 else j + 1)
    assert {float(np.rint(v)) for v in (0.5, 1.5, 2.5)} == {0.0, 2.0}, "rint is ties-to-even"


# ------------------------------------------------------------------------------------------------ rows

OLD = [(s, e) for s in ("ddim", "dpmpp_2m", "tcd") for e in (0.0, 0.5, 1.0)] + [("lcm", 0.0)]


@pytest.mark.parametrize("prediction", ["epsilon", "v"])
@pytest.mark.parametrize("solver,eta", OLD)
def test_old_solver_rows_keep_their_bits(built, solver, eta, prediction):
    lists = [UNEVEN, F.schedule_lcm(4), F.schedule_reference(30), [t for t, _, _ in R.schedule(ALPHAS, 50, 800)], [999], [0]]
    for ts in lists:
        old = built.solver_coefficients(ALPHAS, 0, solver=solver, eta=eta, prediction=prediction, timesteps=ts)
        new = built.solver_rows(ALPHAS, solver, eta, prediction, timesteps=ts)
        assert new.shape == (len(ts), 5) and old.shape == (len(ts), 4)
        assert np.array_equal(np.ascontiguousarray(new[:, [0, 1, 2, 4]]).view(np.uint64), old.view(np.uint64))
        assert not new[:, 3].any(), "c_2 is 0 for the old solvers"
    zt = FC.ZT
    if prediction == "v":
        ts = F.schedule_lcm(4)
        old = built.solver_coefficients(zt, 0, solver=solver, eta=eta, prediction="v", timesteps=ts)
        new = built.solver_rows(zt, solver, eta, "v", timesteps=ts)
        assert np.array_equal(np.ascontiguousarray(new[:, [0, 1, 2, 4]]).view(np.uint64), old.view(np.uint64))


@pytest.mark.parametrize("eta", [0.0, 0.4, 1.0])
def test_restatement_agrees_with_the_literal_loop(eta):
    """the reference checks itself: the alpha / sigma formulas against k-diffusion's loop in its own variables, 1e-12 relative"""
    scheds = [dict(sigmas=L.sigmas_karras(n, ALPHAS)) for n in (1, 2, 3, 8)] + [dict(sigmas=L.sigmas_exponential(8, ALPHAS)), dict(timesteps=UNEVEN),
              dict(timesteps=UNEVEN, t_end=5), C.SCHEDULES["K6e"], dict(sigmas=[10.0, 9.0, 2.0, 1.9, 0.3])]
    for k in scheds:
        lv = L.levels(ALPHAS, **k)
        vp, ve = L.rows_3m_vp(lv, eta), L.rows_3m_ve(lv, eta)
        assert close(vp, ve).all(), (k, vp - ve)


@pytest.mark.parametrize("eta", [0.0, 0.4, 1.0])
def test_3m_rows_against_restatement(built, eta):
    scheds = [dict(sigmas=L.sigmas_karras(n, ALPHAS)) for n in (1, 2, 3, 8)] + [dict(sigmas=L.sigmas_exponential(8, ALPHAS)), dict(timesteps=UNEVEN),
              dict(timesteps=UNEVEN, t_end=5), C.SCHEDULES["K6e"], dict(sigmas=[10.0, 9.0, 2.0, 1.9, 0.3]), dict(sigmas=[10.0, 9.0, 2.0, 1.9, 0.3], sigma_end=0.2)]
    for k in scheds:
        lv = L.levels(ALPHAS, **k)
        got = built.solver_rows(ALPHAS, "dpmpp_3m", eta, **k)
        want = L.rows_3m_vp(lv, eta)
        assert got.shape == want.shape == (len(lv), 5) and close(got, want).all(), (k, got - want)
        assert close(got, L.rows_3m_ve(lv, eta)).all()
        ended = k.get("t_end", -1) >= 0 or k.get("sigma_end", 0.0) > 0.0
        if not ended:
            assert tuple(got[-1]) == (0.0, 1.0, 0.0, 0.0, 0.0), "ap == 1: the iteration returns x0"
        else:
            assert got[-1, 0] > 0.0 and (len(lv) < 3 or got[-1, 3] != 0.0), "a non-zero end level is an ordinary third-order row"
        assert got[0, 2] == 0.0 and got[0, 3] == 0.0, "iteration 0 is first order"
        if len(lv) > 1:
            assert got[1, 3] == 0.0, "iteration 1 is second order"
        assert (got[:, 4] == 0.0).all() if eta == 0.0 else (got[:len(lv) - (0 if ended else 1), 4] > 0.0).all()
    # first order equals DDIM at eta 0 and 2M's first row at any eta
    k = dict(sigmas=L.sigmas_karras(6, ALPHAS))
    assert close(built.solver_rows(ALPHAS, "dpmpp_3m", 0.0, **k)[0], built.solver_rows(ALPHAS, "ddim", 0.0, **k)[0], 1e-11).all()
    assert np.array_equal(built.solver_rows(ALPHAS, "dpmpp_3m", eta, **k)[0], built.solver_rows(ALPHAS, "dpmpp_2m", eta, **k)[0])


@pytest.mark.parametrize("eta", [0.0, 0.4, 1.0])
def test_3m_row_at_zero_alpha_under_v(built, eta):
    ts = [999, 650, 300, 150, 20]
    got = built.solver_rows(FC.ZT, "dpmpp_3m", eta, "v", timesteps=ts)
    want = L.rows_3m_vp(L.levels(FC.ZT, timesteps=ts), eta)
    assert np.isfinite(got).all() and close(got, want).all()
    assert got[0, 2] == got[0, 3] == 0.0 and got[1, 2] == got[1, 3] == 0.0, "the order restarts behind the a == 0 row"
    assert got[2, 2] != 0.0 and got[2, 3] == 0.0 and got[3, 3] != 0.0
    two = built.solver_rows(FC.ZT, "dpmpp_2m", eta, "v", timesteps=ts)
    assert np.array_equal(got[0], two[0]), "the a == 0 row is 2M's limit"
    with pytest.raises(built.InvalidArgument, match="v-prediction"):
        built.solver_rows(FC.ZT, "dpmpp_3m", eta, "epsilon", timesteps=ts)


@pytest.mark.parametrize("solver,eta", [("ddim", 0.0), ("ddim", 1.0), ("dpmpp_2m", 0.0), ("dpmpp_2m", 0.5), ("lcm", 0.0)])
def test_old_solvers_on_sigma_lists(built, solver, eta):
    for name in ("K6", "K6e", "K6r", "E5"):
        k = C.package_schedule(built, name)
        lv = L.levels(ALPHAS, **C.SCHEDULES[name])
        got = built.solver_rows(ALPHAS, solver, eta, **k)
        assert close(got, L.coefficients(lv, solver, eta)).all(), (name, got - L.coefficients(lv, solver, eta))
    # a sigma list made of the integers' sigmas gives the integer list's rows (to the rounding of 1 / (1 + sigma^2)); LCM reads t itself
    ts = F.schedule_reference(4)
    a = built.solver_rows(ALPHAS, solver, eta, sigmas=built.sigma_schedule("of_timesteps", 4, ALPHAS), flags=built.SIGMAS_ROUND_T)
    b = built.solver_rows(ALPHAS, solver, eta, timesteps=ts)
    assert np.abs(a - b).max() <= 1e-9


# ------------------------------------------------------------------------------------------------ refusals

def test_solver_rows_refusals(built):
    l = built.lib()
    out = np.full(5 * 16, 7.25, dtype=np.float64)
    po = out.ctypes.data_as(ctypes.c_void_p)
    K6 = L.sigmas_karras(6, ALPHAS)

    def call(solver=built.SOLVER_DPMPP_3M, prediction=0, eta=0.0, o=po, cap=16, alphas=ALPHAS, **k):
        desc, keep, n = built._schedule_desc(alphas, **k)
        return l.sdxl_solver_rows(ctypes.byref(desc), solver, prediction, ctypes.c_double(eta), o, cap), l.sdxl_last_error().decode()

    bad = [(dict(sigmas=[1.0, 2.0]), "sigmas"), (dict(sigmas=[2.0, 2.0]), "sigmas"), (dict(sigmas=[2.0, 0.0]), "sigmas"), (dict(sigmas=[2.0, -1.0]), "sigmas"),
           (dict(sigmas=[float("inf"), 1.0]), "sigmas"), (dict(sigmas=[float("nan")]), "sigmas"), (dict(sigmas=K6, sigma_end=K6[-1]), "sigmas"),
           (dict(sigmas=K6, sigma_end=-0.1), "sigmas"), (dict(sigmas=K6, sigma_end=float("nan")), "sigmas"), (dict(sigmas=K6, flags=2), "sigmas"),
           (dict(sigmas=K6, solver=built.SOLVER_TCD, eta=0.3), "sigmas"), (dict(sigmas=K6, solver=built.SOLVER_LCM, eta=0.3), "eta"),
           (dict(timesteps=UNEVEN, t_end=20), "timesteps"), (dict(timesteps=UNEVEN, t_end=-2), "timesteps"), (dict(timesteps=UNEVEN, t_end=900), "timesteps"),
           (dict(timesteps=[20, 300]), "timesteps"), (dict(timesteps=UNEVEN, sigmas=K6), "exactly one"), (dict(), "exactly one"),
           (dict(sigmas=K6, solver=2), "solver"), (dict(sigmas=K6, solver=7), "solver"), (dict(sigmas=K6, solver=-1), "solver"),
           (dict(sigmas=K6, eta=1.5), "eta"), (dict(sigmas=K6, prediction=5), "prediction"), (dict(sigmas=K6, cap=5), "capacity"),
           (dict(timesteps=[999, 500], alphas=FC.ZT), "v-prediction")]
    for kw, word in bad:
        rc, msg = call(**kw)
        assert rc == 1 and word in msg, (kw, rc, msg)
        assert (out == 7.25).all(), f"{kw}: out was written"
    assert l.sdxl_solver_rows(None, 5, 0, ctypes.c_double(0.0), po, 16) == 1 and (out == 7.25).all()
    desc, keep, n = built._schedule_desc(ALPHAS, sigmas=K6)
    assert l.sdxl_solver_rows(ctypes.byref(desc), 5, 0, ctypes.c_double(0.0), None, 16) == 1
    rc, msg = call(sigmas=K6, cap=6)
    assert rc == 0 and (out[:30] != 7.25).any() and (out[30:] == 7.25).all()


def test_old_entries_refuse_the_new_solver(built):
    l = built.lib()
    a = np.ascontiguousarray(ALPHAS, dtype=np.float32)
    pa = a.ctypes.data_as(ctypes.c_void_p)
    out = np.full(4 * 16, 7.25, dtype=np.float64)
    po = out.ctypes.data_as(ctypes.c_void_p)
    ts = np.ascontiguousarray(UNEVEN, dtype=np.int32)
    for rc in (l.sdxl_solver_coefficients_ts(pa, 1000, ts.ctypes.data_as(ctypes.c_void_p), 4, 5, 0, ctypes.c_double(0.0), po, 16),
               l.sdxl_solver_coefficients_pred(pa, 1000, 4, 0, 5, 0, ctypes.c_double(0.0), po, 16),
               l.sdxl_solver_coefficients(pa, 1000, 4, 0, 5, ctypes.c_double(0.0), po, 16)):
        msg = l.sdxl_last_error().decode()
        assert rc == 1 and "sdxl_solver_rows" in msg and "sdxl_sampler_step_replay_levels" in msg and "solver" in msg
        assert (out == 7.25).all()


def test_sigma_entry_refusals(built):
    l = built.lib()
    a = np.ascontiguousarray(ALPHAS, dtype=np.float32)
    pa = a.ctypes.data_as(ctypes.c_void_p)
    out = np.full(64, -7.0, dtype=np.float64)
    po = out.ctypes.data_as(ctypes.c_void_p)
    call = lambda kind=0, n=6, al=pa, nt=1000, lo=0.0, hi=0.0, rho=7.0, o=po, cap=64: l.sdxl_sigma_schedule(kind, n, al, nt, lo, hi, rho, o, cap)
    zt = np.ascontiguousarray(FC.ZT, dtype=np.float32)
    bad = [dict(kind=3), dict(kind=-1), dict(n=0), dict(n=1001), dict(al=None), dict(nt=1), dict(lo=2.0, hi=1.0), dict(lo=1.0, hi=1.0), dict(rho=0.0),
           dict(rho=float("nan")), dict(hi=float("inf")), dict(o=None), dict(cap=5), dict(kind=2, n=30, cap=30), dict(al=zt.ctypes.data_as(ctypes.c_void_p)),
           dict(kind=2, n=4, al=zt.ctypes.data_as(ctypes.c_void_p))]
    for kw in bad:
        assert call(**kw) == 1 and l.sdxl_last_error().decode(), kw
        assert (out == -7.0).all(), f"{kw}: out was written"
    assert call(cap=6) == 6 and (out[:6] > 0).all() and (out[6:] == -7.0).all()
    t = ctypes.c_double(-7.0)
    for kw in (dict(s=0.0), dict(s=-1.0), dict(s=float("nan")), dict(s=float("inf")), dict(f=2), dict(al=None), dict(nt=1)):
        rc = l.sdxl_sigma_to_timestep(kw.get("al", pa), kw.get("nt", 1000), kw.get("s", 1.0), kw.get("f", 0), ctypes.byref(t))
        assert rc == 1 and l.sdxl_last_error().decode() and t.value == -7.0, kw
    assert l.sdxl_sigma_to_timestep(pa, 1000, 1.0, 0, None) == 1
    for kw in (dict(kind="cosine", n_steps=4), dict(kind="karras", n_steps=0), dict(kind="karras", n_steps=4, rho=-1.0)):
        with pytest.raises(built.InvalidArgument):
            built.sigma_schedule(**kw)


# ------------------------------------------------------------------------------------------------ the bound of the kernel test

@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_fp32_emulation_stays_inside_the_kernel_bound(case):
    """the noise the device would draw is played by seeded numpy normals here: the bound does not depend on which unit normals they are"""
    solver, shape = case[0], case[8]
    n, h, w = shape
    inp = S.make_inputs(shape)
    rng = np.random.default_rng(5)
    z = rng.standard_normal((2, S.MAX_ITERS, n, 4, h, w)).astype(np.float32).astype(np.float64)
    lv, table, rows, kw = C.reference_args(case, inp, lambda i: z[0, i], lambda i: z[1, i], lambda r, scales, phi: FC.rescale_factors_f64(r, n, scales, phi))
    ref, M, hist, hist2 = L.replay(lv, solver, table, rows.astype(np.float64), inp["latent0"].astype(np.float64), **kw)
    got = L.emulate_f32(lv, solver, table, rows, inp["latent0"], **kw).astype(np.float64)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    worst = 0.0
    for i in range(len(lv) + 1):
        err, bound = float(np.abs(got[i] - ref[i]).max()), L.U * C.ROUNDINGS * (i + 1) * M[i]
        worst = max(worst, err / bound if bound else (0.0 if err == 0.0 else np.inf))
        assert err <= bound, f"latent {i}: emulation error {err:.3e} over the bound {bound:.3e} (M {M[i]:.3f})"
    print(f"{C.case_id(case)}: fp32 emulation, worst error / bound {worst:.3f}, M {M[-1]:.2f}")
    assert not ref[-1].std() == 0.0


def test_case_table_covers_what_it_must():
    m3 = [c for c in C.CASES if c[0] == "dpmpp_3m"]
    assert {(c[7], c[1]) for c in m3} >= {("K6", 0.0), ("K6", 1.0), ("U4", 0.0), ("U4", 1.0)}
    assert {c[2] for c in m3} == {"epsilon", "v"} and {c[4] for c in m3} == {"scalar", "single", "scales", "interval", "all"}
    assert {c[5] for c in m3} == {False, True} and {c[6] for c in m3} == {False, True} and {c[9] for c in m3} == {False, True}
    assert all(c[1] == 0.0 for c in C.CASES if not c[9]), "explicit noise runs at eta 0"
    assert {c[8] for c in m3} == set(S.SHAPES) and {"K6e", "U4e"} <= {c[7] for c in m3}
    assert {c[0] for c in C.CASES if "sigmas" in C.SCHEDULES[c[7]]} == {"dpmpp_3m", "dpmpp_2m", "lcm", "ddim"}
    assert len(C.SCHEDULES["K6"]["sigmas"]) == 6 and C.SCHEDULES["U4"]["timesteps"] == UNEVEN and FC.ZT[999] == 0.0
    # a 6-entry 3M table reaches third order, and its last-but-one rows read both histories
    t = L.rows_3m_vp(L.levels(ALPHAS, **C.SCHEDULES["K6"]), 1.0)
    assert (t[2:5, 3] != 0.0).all() and (t[1:5, 2] != 0.0).all()


def test_python_names(built):
    assert built.SOLVER_DPMPP_3M == L.DPMPP_3M == 5 and built.SIGMAS_ROUND_T == 1
    for name in ("sdxl_diffuser_set_sigmas", "sdxl_diffuser_get_sigmas", "sdxl_diffuser_set_timesteps_end", "sdxl_sigma_schedule", "sdxl_sigma_to_timestep",
                 "sdxl_continue_latent", "sdxl_solver_rows", "sdxl_sampler_step_replay_levels"):
        assert name in built.ABI_SYMBOLS and hasattr(built.lib(), name)
