"""tests/vae_block_ref.py checked against itself on the CPU, on the very operands tests/test_gpu_vae_blocks.py sends to the GPU (the two-pass cases at
their subset rows): each mode's emulation is finite, reproducible and inside the error class of its mode, and every planted defect lands at least 5 x
outside the bound (margin x the emulation's own error against fp64) of every case and mode it applies to -- or turns the output non-finite.  So a GPU
result inside those bounds rules the planted defects out.

Measured here (error / bound of the defective emulation; the clean emulations sit at 1 / margin by construction):
  attention, f32 / split: scale_quarter 2.2e4 ... 3.0e5, norm_256 1.3e6 ... 1.2e7 (split, peaked cases: non-finite, the unnormalised P overflows f16),
    pass_offset 7.8e3 ... 1.4e5, pv_tail 2.3e3 ... 1.7e5, batch_keys 1.2e5 ... 1.9e5; split only: p_lo_dropped 12.7 ... 56, p_noscale 8.3 (flat case;
    0.3 ... 0.5 on the peaked cases, where it is not held to the factor: vae_block_ref.attn_defect_applies).
  attention, f16: scale_quarter 353 ... 503, norm_256 8.6e3 ... 2.1e4, pass_offset 230, pv_tail 22 ... 239, batch_keys 358 ... 453.
  res block, split, magnitude case (per entry): one_scale (0.25, 155) -- the entry that is scaled by its neighbour's maximum is the one that loses --,
    no_a_scale (1.1e6, 3.2e10), absmax_no_last_row non-finite in both."""
import math

import pytest
import torch

import vae_block_ref as R

FACTOR = 5.0


@pytest.mark.parametrize("name", [c[0] for c in R.ATTN_CASES])
def test_attention_emulations_are_consistent_and_defects_leave_the_bounds(name):
    errs = {}
    for mode in R.attn_modes(name):
        clean = R.attn_emulate(name, mode)
        bound, e = R.attn_bound(name, mode)
        errs[mode] = e
        assert torch.isfinite(clean).all() and 0.0 < e < math.inf
        assert torch.equal(clean, R.attn_emulate(name, mode)), "the emulation is a function of its operands"
        assert clean.shape == R.attn_ref(name)[0].shape
        for defect in R.ATTN_DEFECTS:
            if not R.attn_defect_applies(defect, name, mode):
                continue
            r = R.attn_error(R.attn_emulate(name, mode, defect), name) / bound
            print(f"attn {name} {mode} {defect}: {r:.3g} x bound")
            assert r >= FACTOR, (name, mode, defect, r)
    # the classes: fp32 and split agree with fp64 to fp32 rounding of a C- and HW-long chain, f16 to operand rounding (2^-11 per operand)
    assert errs["f32"] < 2e-5 and errs["split"] < 2e-5
    if "f16" in errs:
        assert 20 * errs["split"] < errs["f16"] < 2e-2


def test_attention_defects_change_nothing_where_they_do_not_apply_by_shape():
    # (a defect that cannot show at a shape must leave the clean bits: what attn_defect_applies says about shapes is what the emulation does)
    assert torch.equal(R.attn_emulate("base_8x8", "f32", "pv_tail"), R.attn_emulate("base_8x8", "f32"))
    assert torch.equal(R.attn_emulate("base_8x8", "f32", "norm_256"), R.attn_emulate("base_8x8", "f32"))
    assert torch.equal(R.attn_emulate("wide_24x40", "f32", "pass_offset"), R.attn_emulate("wide_24x40", "f32"))
    assert torch.equal(R.attn_emulate("ragged_9x9", "split", "batch_keys"), R.attn_emulate("ragged_9x9", "split"))


def test_subset_rows_straddle_the_pass_boundary():
    rows = R.subset_rows(90 * 92)
    assert len(rows) == 64 + 64 + 152 and rows[0] == 0 and rows[-1] == 8279
    assert (rows < R.QT).sum() == 64 + 64 + 64 and (rows >= R.QT).sum() == 88 and {8191, 8192} <= set(rows.tolist())
    assert len(R.subset_rows(960)) == 960


@pytest.mark.parametrize("name", [c[0] for c in R.RES_CASES])
def test_res_block_emulations_are_consistent_and_defects_leave_the_bounds(name):
    mag = R.res_case(name)[6]
    errs = {}
    for mode in ("f32", "split") if mag else ("f32", "f16", "split"):
        clean = R.res_emulate(name, mode)
        bounds, e = R.res_bounds(name, mode)
        errs[mode] = max(e)
        assert torch.isfinite(clean).all() and all(0.0 < v < math.inf for v in e)
        assert torch.equal(clean, R.res_emulate(name, mode)) and clean.shape == R.res_ref(name).shape
        for defect in R.RES_DEFECTS:
            if not R.res_defect_applies(defect, name, mode):
                continue
            r = [v / b for v, b in zip(R.res_errors(R.res_emulate(name, mode, defect), name), bounds)]
            print(f"res {name} {mode} {defect}: {', '.join(f'{v:.3g}' for v in r)} x bound per entry")
            # (the scale defects may show as a non-finite output or a result >= 2 x off instead: inf and ratios of 1e6 are both far past the factor)
            assert max(r) >= FACTOR, (name, mode, defect, r)
    assert errs["f32"] < 5e-6 and errs["split"] < 5e-6
    if "f16" in errs:
        assert 20 * errs["split"] < errs["f16"] < 1e-2


def test_magnitude_case_is_what_the_shortcut_defects_need():
    d = R.res_inputs("magnitude_16x24")
    x = d["x"]
    for b, e in ((0, 15), (1, -7)):
        top = float(x[b].abs().max())
        assert float(x[b, -1, -1, -1].abs()) == top                                   # the largest element sits at the last pixel of the last channel
        assert top >= 7.9 * float(x[b].abs().flatten()[:-1].max())                     # 8 x the rest: an absmax that misses it overflows f16
    assert float(x[0].abs().max() / x[1].abs().max()) > 2.0 ** 21                     # the entries differ by ~2^22: one scale cannot serve both
    ref = R.res_ref("magnitude_16x24")
    assert float(ref[0].abs().max()) > 2.0 ** 15 and float(ref[1].abs().max()) < 1.0
