"""The evidence that tests/test_gpu_conditioning.py would notice a subtly wrong GEMV / timestep-embedding kernel, without running anything broken on a
GPU: on the very operands the GPU tests use, a CPU emulation of the kernel's fp32 arithmetic (gemv_ref.gemv_emulate) lies well inside the derived
bound, and the same emulation with one planted defect -- a dropped product, a skipped partial k-iteration, a chunk launched without its row offset, an
ignored SiLU flag, a shifted output column -- lies outside it.

A defect is asserted on every case where it changes what the kernel computes (gemv_ref.defect_applies: a row-offset defect needs a second launch, a
skipped partial iteration a K that is no multiple of the wavefront step, ...); where it changes nothing there is nothing to notice.
test_every_defect_is_noticed_somewhere pins which cases those are, so a change of the case list cannot quietly lose one."""
import numpy as np
import pytest

import gemv_ref as R

PAIRS = [(c, f16) for c in R.GEMV_CASES for f16 in (False, True)]
IDS = [f"{c[0]}-{'f16' if f16 else 'f32'}" for c, f16 in PAIRS]

_cache = {}


def _case(case, f16):
    """(operands, fp64 reference, bound, clean emulation) of a case: computed once, shared by the tests below, never modified"""
    key = (case[0], f16)
    if key not in _cache:
        _, K, N, Bm, flags = case
        d = R.make_case(K, N, Bm, flags, f16)
        y, bound = R.gemv_ref(**d)
        _cache[key] = (d, y, bound, R.gemv_emulate(**d))
    return _cache[key]


def _ratio(out, y, bound):
    return float((np.abs(out.astype(np.float64) - y) / bound).max())


@pytest.mark.parametrize("case,f16", PAIRS, ids=IDS)
def test_clean_emulation_is_inside_the_bound(case, f16):
    d, y, bound, clean = _case(case, f16)
    r = _ratio(clean, y, bound)
    print(f"{case[0]} {'f16' if f16 else 'f32'}: clean emulation worst error / bound {r:.3f}")
    assert np.isfinite(clean).all() and (bound > 0).all()
    assert r <= 1.0


@pytest.mark.parametrize("case,f16", PAIRS, ids=IDS)
def test_every_planted_defect_leaves_the_bound(case, f16):
    d, y, bound, clean = _case(case, f16)
    _, K, N, Bm, flags = case
    for defect in R.DEFECTS:
        if not R.defect_applies(defect, K, Bm, d["yadd"] is not None, d["silu_in"], d["silu_out"], f16):
            assert np.array_equal(R.gemv_emulate(**d, defect=defect), clean), defect      # nothing to notice here
            continue
        r = _ratio(R.gemv_emulate(**d, defect=defect), y, bound)
        print(f"{case[0]} {'f16' if f16 else 'f32'} {defect}: worst error / bound {r:.1f}")
        assert r >= (100.0 if defect in R.TAIL_DEFECTS else 1.0), (defect, r)


def test_every_defect_is_noticed_somewhere():
    seen = {d: [] for d in R.DEFECTS}
    for (name, K, N, Bm, flags), f16 in PAIRS:
        for d in R.DEFECTS:
            if R.defect_applies(d, K, Bm, "a" in flags, "i" in flags, "o" in flags, f16):
                seen[d].append((name, f16))
    assert all(seen[d] for d in R.DEFECTS), seen
    # the launcher's chunking as the issue states it: 5 rows per launch at K = 2816, 6 at K = 2560, 8 at small K, 1 at the 64 KiB limit, none beyond
    assert [R.rows_per_launch(k, False) for k in (2816, 2560, 64, 16384, 16385)] == [5, 6, 8, 1, 0]
    assert [R.rows_per_launch(k, True) for k in (2816, 2560, 64, 16384, 16385)] == [5, 6, 8, 1, 0]
    # a partial last iteration at SDXL widths exists in f16 (K = 1280: 2.5 steps of 512, K = 2816: 5.5) and at the odd small K in both
    assert ("time_lin2_b8", True) in seen["skip_partial_iter"] and ("label_base_b8", True) in seen["skip_partial_iter"]
    assert ("k_and_n_tails", False) in seen["skip_partial_iter"] and ("time_lin1_b8", False) in seen["skip_partial_iter"]
    # row offsets of a second launch: X on 5+1, 5+3, 6+1, 8+1 and 1+1 rows, Yadd with 5+3
    assert {n for n, _ in seen["x_no_offset"]} == {"label_base_b6", "label_base_b8", "label_refiner_b7", "chunks_of_8", "staging_limit",
                                                   "all_flags_null_bias_two_launches"}
    assert {n for n, _ in seen["yadd_no_offset"]} == {"all_flags_null_bias_two_launches"}


def test_emulation_refuses_what_the_launcher_refuses():
    d = R.make_case(16385, 8, 1, "", False)
    with pytest.raises(ValueError):
        R.gemv_emulate(**d)


@pytest.mark.parametrize("dim", R.TEMB_DIMS)
def test_timestep_embedding_bound(dim):
    for t in (R.TEMB_T, R.TEMB_T[4:5]):
        ref, bound = R.temb_ref(t, dim)
        r = _ratio(R.temb_emulate(t, dim), ref, bound)
        print(f"temb dim {dim} n {len(t)}: fp32 numpy worst error / bound {r:.3f}")
        assert r <= 1.0
        for defect in ("swap", "dim_for_half", "j_plus_1"):
            assert _ratio(R.temb_emulate(t, dim, defect), ref, bound) > 100.0, defect
    ref0, _ = R.temb_ref([0.0], dim)
    assert (ref0[:, :dim // 2] == 1.0).all() and (ref0[:, dim // 2:] == 0.0).all()
    # the high-frequency end is where a global tolerance hides errors: at t = 1, j = half - 1 the bound is far below 2e-4
    _, b1 = R.temb_ref([1.0], dim)
    assert b1[0, dim // 2 - 1] < 2e-4 / 500
