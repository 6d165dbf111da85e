"""Few-step sampling, host logic (no device): the timestep spacings, the list form of the coefficient table, the LCM and TCD rows against
the fp64 restatement of tests/fewstep_ref.py, the argument errors, and the check that the bound of tests/test_gpu_fewstep_step.py is a
condition the kernel's arithmetic meets (an fp32 numpy emulation of its lines, on that test's inputs)."""
import ctypes
import os

import numpy as np
import pytest

import fewstep_cases as C
import fewstep_ref as F
import sampler_step_cases as S
import solver_ref as R
from oracle import config as OC

ALPHAS = OC.alphas_cumprod()
REL = 1e-12                  # tests/test_cpu_solver.py's bar and reasoning: both sides are f64 evaluations of the same short expressions
N_STEPS = [1, 2, 3, 4, 7, 8, 30, 50]
UNEVEN = [[999, 759, 499, 259], [900, 650, 300, 20]]


@pytest.fixture(scope="module")
def built(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg


def close(got, want):
    return np.abs(got - want) <= REL * np.abs(want)


# ------------------------------------------------------------------------------------------------ spacings

@pytest.mark.parametrize("n_steps", N_STEPS)
@pytest.mark.parametrize("kind", ["reference", "trailing", "leading", "lcm"])
def test_schedule_against_restatement(built, kind, n_steps):
    got = built.timestep_schedule(kind, n_steps)
    assert got == F.timestep_schedule(kind, n_steps)
    assert all(0 <= t < 1000 for t in got) and all(b < a for a, b in zip(got, got[1:]))
    if kind == "reference":
        assert len(got) == built.step_count(n_steps, 0, 1000)
        assert got == [t for t, _, _ in R.schedule(ALPHAS, n_steps)]
    else:
        assert len(got) == n_steps


def test_known_lists(built):
    assert built.timestep_schedule("trailing", 4) == [999, 749, 499, 249]
    assert built.timestep_schedule("leading", 4, offset=1) == [751, 501, 251, 1]
    assert built.timestep_schedule("lcm", 4, origin_steps=50) == [999, 759, 499, 259]
    assert built.timestep_schedule("lcm", 8) == [999, 879, 759, 639, 499, 379, 259, 139]
    assert len(built.timestep_schedule("reference", 30)) == 31
    assert built.timestep_schedule(built.SCHEDULE_LCM, 4) == built.timestep_schedule("lcm", 4)


def test_schedule_refusals(built):
    l = built.lib()
    out = np.full(64, -7, dtype=np.int32)
    po = out.ctypes.data_as(ctypes.c_void_p)
    call = lambda kind=3, n_steps=4, n_train=1000, param=50, o=po, cap=64: l.sdxl_timestep_schedule(kind, n_steps, n_train, param, o, cap)
    bad = [dict(n_steps=51), dict(param=0), dict(param=1001), dict(kind=2, param=250), dict(kind=2, param=-1), dict(cap=3), dict(kind=4),
           dict(kind=-1), dict(n_steps=0), dict(n_steps=1001), dict(o=None), dict(n_train=0), dict(kind=0, n_steps=30, cap=30)]
    for kw in bad:
        assert call(**kw) == 1 and l.sdxl_last_error().decode(), kw
        assert (out == -7).all(), f"{kw}: out was written"
    assert call(kind=2, param=249) == 4 and list(out[:4]) == [999, 749, 499, 249] and (out[4:] == -7).all()
    assert call(cap=4) == 4
    for kw in (dict(kind="karras", n_steps=4), dict(kind="lcm", n_steps=51), dict(kind="leading", n_steps=4, offset=250)):
        with pytest.raises(built.InvalidArgument):
            built.timestep_schedule(**kw)


# ------------------------------------------------------------------------------------------------ the table on a list

@pytest.mark.parametrize("prediction", ["epsilon", "v"])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_reference_list_gives_the_same_bits(built, solver, eta, prediction):
    for n_steps, step_start in [(4, 0), (30, 0), (50, 800), (7, 0)]:
        ts = [t for t, _, _ in R.schedule(ALPHAS, n_steps, step_start)]
        old = built.solver_coefficients(ALPHAS, n_steps, step_start, solver=solver, eta=eta, prediction=prediction)
        new = built.solver_coefficients(ALPHAS, 0, 0, solver=solver, eta=eta, prediction=prediction, timesteps=ts)
        assert old.shape == new.shape == (len(ts), 4)
        assert np.array_equal(old.view(np.uint64), new.view(np.uint64))


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("ts", UNEVEN, ids=["lcm4", "hand"])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_uneven_list_against_restatement(built, solver, ts, eta):
    got = built.solver_coefficients(ALPHAS, 0, solver=solver, eta=eta, timesteps=ts)
    want = F.coefficients(ALPHAS, ts, solver, eta)
    assert got.shape == want.shape == (4, 4) and close(got, want).all(), got - want
    if solver == "dpmpp_2m":
        assert got[0, 2] == 0.0 and (got[1:-1, 2] < 0.0).all() and tuple(got[-1]) == (0.0, 1.0, 0.0, 0.0)


LISTS = UNEVEN + [[999], [0], F.schedule_lcm(8), F.schedule_trailing(4), F.schedule_leading(4), F.schedule_reference(30)]


@pytest.mark.parametrize("ts", LISTS, ids=lambda ts: f"{len(ts)}from{ts[0]}")
def test_lcm_rows(built, ts):
    got = built.solver_coefficients(ALPHAS, 0, solver="lcm", timesteps=ts)
    want = F.lcm_rows(ALPHAS, ts)
    assert close(got, want).all(), got - want
    s = 10.0 * ts[-1]
    assert np.abs(got[-1] - np.array([0.25 / (s * s + 0.25), s / np.sqrt(s * s + 0.25), 0.0, 0.0])).max() <= REL, "the last row is (c_skip, c_out, 0, 0)"
    assert (got[:, 2] == 0.0).all() and (got[:, 3] >= 0.0).all() and (got[:, 3] <= 1.0).all() and (np.abs(got[:, 0]) <= 1.0).all()
    assert (got[:-1, 3] > 0.0).all(), "every iteration but the last re-noises"
    # without a list the solver runs on the reference's rule
    assert np.array_equal(built.solver_coefficients(ALPHAS, 4, solver="lcm"), built.solver_coefficients(ALPHAS, 0, solver="lcm", timesteps=F.schedule_reference(4)))


@pytest.mark.parametrize("gamma", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("ts", LISTS, ids=lambda ts: f"{len(ts)}from{ts[0]}")
def test_tcd_rows(built, ts, gamma):
    got = built.solver_coefficients(ALPHAS, 0, solver="tcd", eta=gamma, timesteps=ts)
    want = F.tcd_rows(ALPHAS, ts, gamma)
    assert close(got, want).all(), got - want
    assert tuple(got[-1]) == (0.0, 1.0, 0.0, 0.0), "the last iteration returns x0"
    assert (got[:, 2] == 0.0).all() and (got[:, 3] >= 0.0).all() and (got[:, 3] <= 1.0).all() and (np.abs(got[:, 0]) <= 1.0).all()
    if gamma == 0.0:
        ddim = built.solver_coefficients(ALPHAS, 0, solver="ddim", eta=0.0, timesteps=ts)
        assert close(got[:-1], ddim[:-1]).all() and (got[:, 3] == 0.0).all(), "gamma = 0 is DDIM at eta 0"
        assert np.abs(got[-1] - ddim[-1]).max() <= REL
    else:
        assert (got[:-1, 3] > 0.0).all()


def test_rows_under_v_at_zero_alpha(built):
    ts = F.schedule_lcm(4)
    for solver, gamma in (("lcm", 0.0), ("tcd", 0.3), ("tcd", 1.0)):
        got = built.solver_coefficients(C.ZT, 0, solver=solver, eta=gamma, prediction="v", timesteps=ts)
        assert np.isfinite(got).all() and close(got, F.coefficients(C.ZT, ts, solver, gamma)).all()
        with pytest.raises(built.InvalidArgument, match="v-prediction"):
            built.solver_coefficients(C.ZT, 0, solver=solver, eta=gamma, prediction="epsilon", timesteps=ts)


# ------------------------------------------------------------------------------------------------ the bound of the kernel test

@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_fp32_emulation_stays_inside_the_kernel_bound(case):
    """the noise the device would draw is played by seeded numpy normals here: the bound does not depend on which unit normals they are"""
    shape = case[8]
    n, h, w = shape
    inp = S.make_inputs(shape)
    rng = np.random.default_rng(5)
    z = rng.standard_normal((2, S.MAX_ITERS, n, 4, h, w)).astype(np.float32).astype(np.float64)
    alphas, ts, table, rows, kw = C.reference_args(case, inp, lambda i: z[0, i], lambda i: z[1, i],
                                                   lambda r, scales, phi: C.rescale_factors_f64(r, n, scales, phi))
    ref, M = F.replay(alphas, ts, table, rows.astype(np.float64), inp["latent0"].astype(np.float64), **kw)
    got = F.emulate_f32(alphas, ts, table, rows, inp["latent0"], **kw).astype(np.float64)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    worst = 0.0
    for i in range(len(ts) + 1):
        err, bound = float(np.abs(got[i] - ref[i]).max()), F.U * 8 * (i + 1) * M[i]
        worst = max(worst, err / bound if bound else (0.0 if err == 0.0 else np.inf))
        assert err <= bound, f"latent {i}: emulation error {err:.3e} over the bound {bound:.3e} (M {M[i]:.3f})"
    print(f"{C.case_id(case)}: fp32 emulation, worst error / bound {worst:.3f}, M {M[-1]:.2f}")
    assert not ref[-1].std() == 0.0


def test_case_table_covers_every_column():
    for solver in ("lcm", "tcd"):
        rows = [c for c in C.CASES if c[0] == solver]
        assert {c[2] for c in rows} == {"epsilon", "v"} and {c[3] for c in rows} == {False, True}
        assert {c[4] for c in rows} == {"scalar", "single", "scales", "interval", "all"}
        assert {c[5] for c in rows} == {False, True} and {c[6] for c in rows} == {False, True} and {c[9] for c in rows} == {False, True}
        assert {len(C.LISTS[c[7]]) for c in rows} == {1, 4, 8} and {c[8] for c in rows} == set(S.SHAPES)
        assert all(C.LISTS[c[7]][0] == 999 for c in rows if c[3]), "the zero-terminal cases start at a == 0"
    assert {c[1] for c in C.CASES if c[0] == "tcd"} == {0.0, 0.3, 1.0} and {c[1] for c in C.CASES if c[0] == "lcm"} == {0.0}
    assert C.ZT[999] == 0.0


# ------------------------------------------------------------------------------------------------ argument errors

def test_argument_errors(built):
    l = built.lib()
    a = np.ascontiguousarray(ALPHAS, dtype=np.float32)
    pa = a.ctypes.data_as(ctypes.c_void_p)
    out = np.full(4 * 16, 7.25, dtype=np.float64)
    po = out.ctypes.data_as(ctypes.c_void_p)

    def call(ts=(999, 759, 499, 259), alphas=pa, n_train=1000, solver=built.SOLVER_TCD, prediction=0, eta=0.0, o=po, cap=16, n=None):
        t = np.ascontiguousarray(ts, dtype=np.int32) if ts is not None else None
        return l.sdxl_solver_coefficients_ts(alphas, n_train, t.ctypes.data_as(ctypes.c_void_p) if t is not None else None,
                                             len(ts) if n is None else n, solver, prediction, ctypes.c_double(eta), o, cap)

    lists = [dict(ts=(999, 999, 499)), dict(ts=(259, 499)), dict(ts=(1000, 500)), dict(ts=(500, -1)), dict(ts=None, n=4), dict(n=0), dict(n=-2),
             dict(ts=tuple(range(1000, -1, -1)))]
    for kw in lists:
        assert call(**kw) == 1 and "timesteps" in l.sdxl_last_error().decode(), kw
        assert (out == 7.25).all(), f"{kw}: out was written"
    other = [dict(solver=7), dict(solver=2), dict(solver=-1), dict(eta=1.5), dict(eta=float("nan")), dict(cap=3), dict(alphas=None), dict(o=None),
             dict(prediction=5), dict(solver=built.SOLVER_LCM, eta=0.5), dict(n_train=0)]
    for kw in other:
        assert call(**kw) == 1 and l.sdxl_last_error().decode(), kw
        assert (out == 7.25).all(), f"{kw}: out was written"
    assert call(solver=7) == 1 and "solver" in l.sdxl_last_error().decode()
    assert call(solver=built.SOLVER_LCM, eta=0.5) == 1 and "eta" in l.sdxl_last_error().decode()
    assert call(cap=4) == 0 and (out[:16] != 7.25).any() and (out[16:] == 7.25).all()
    with pytest.raises(built.InvalidArgument, match="timesteps"):
        built.solver_coefficients(ALPHAS, 0, solver="lcm", timesteps=[259, 499])
    with pytest.raises(built.InvalidArgument, match="eta"):
        built.solver_coefficients(ALPHAS, 0, solver="lcm", eta=0.3, timesteps=[999, 499])
    with pytest.raises(built.EngineError):
        built.solver_coefficients(ALPHAS, 0, solver="euler", timesteps=[999, 499])


def test_python_names(built):
    assert (built.SOLVER_LCM, built.SOLVER_TCD) == (F.LCM, F.TCD)
    assert np.array_equal(built.solver_coefficients(ALPHAS, 0, solver="tcd", eta=0.3, timesteps=[999, 499]),
                          built.solver_coefficients(ALPHAS, 0, solver=built.SOLVER_TCD, eta=0.3, timesteps=[999, 499]))
    for name in ("sdxl_diffuser_set_timesteps", "sdxl_diffuser_get_timesteps", "sdxl_timestep_schedule", "sdxl_solver_coefficients_ts",
                 "sdxl_sampler_step_replay_ts"):
        assert name in built.ABI_SYMBOLS and hasattr(built.lib(), name)
