"""tests/unet_block_ref.py on the CPU: the fp64 reference against the fp32 oracle, every clean emulation inside its own bound, and every planted
defect over the bound of the case it is planted on.  Figures are printed first (pytest -s)."""
import pytest
import torch

import unet_block_ref as R
from oracle import model as OM

CASE_NAMES = [c[0] for c in R.CASES + R.RF_CASES]
# fp32 against fp64: a GEMM of depth K leaves about sqrt(K) 2^-24 relative (random-walk accumulation; K <= 27648, the refiner's 3072-wide convolutions:
# sqrt(27648) 2^-24 = 9.9e-6; the base's K <= 23040: 9e-6), a chain has at most 22 of them (either middle block at depth 2: 4 convolutions + 2 x 8
# projections + proj_in / proj_out) adding in quadrature: sqrt(22) 9.9e-6 = 4.7e-5 if every one of them had the longest K (the deepest chain with a
# K = 27648 member has four GEMMs) -- the constant that K <= 23040 gave (4.3e-5 -> 5e-5) still holds
FP32_TOL = 5e-5


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fp64_reference_agrees_with_fp32_oracle(name):
    out = R.oracle32(name)
    assert out.dtype == torch.float32
    errs = R.errors(out, name)
    print(f"unet_block_ref {name}: fp32 oracle against fp64 {['%.3e' % e for e in errs]}")
    assert max(errs) < FP32_TOL
    # the f32 emulation restates the oracle with the engine's accumulation chain: fp32 accuracy as well
    emu = R.emulation_errors(name, 0)
    print(f"  f32 emulation {['%.3e' % e for e in emu]}")
    assert max(emu) < FP32_TOL


@pytest.mark.parametrize("name", ["rest_640_skip", "out_960_res"])
def test_f16_emulation_restates_the_oracles_operands_emulation(name):
    # dtype 2 is the oracle's `operands` emulation with every class on + the f16 store of conv_in's output: both within a factor of two of each other
    classes = ("qkv", "attn", "out", "xattn", "geglu", "ff", "conv")
    OM.NUM.set("operands", classes)
    try:
        ora = R.errors(R._oracle(name, *R.inputs(name), R.weights(name)), name)
    finally:
        OM.NUM.set(None)
    emu = R.emulation_errors(name, 2)
    print(f"unet_block_ref {name}: oracle operands emulation {['%.3e' % e for e in ora]}  dtype 2 emulation {['%.3e' % e for e in emu]}")
    assert all(0.5 * o <= e <= 2.0 * o for e, o in zip(emu, ora))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_clean_emulations_sit_inside_their_bounds(name):
    # the bound comes from input seed 0; the emulation on two further seeds of the case (other x, emb, context; their own fp64 references) must sit
    # inside it as well: a margin that did not cover the emulation's own spread would need deriving from that spread (module docstring)
    for dtype in R.case_dtypes(name):
        bnd, emu = R.bounds(name, dtype)
        print(f"unet_block_ref {name} dtype {dtype}: emulation {['%.3e' % e for e in emu]}  bound {['%.3e' % b for b in bnd]}")
        assert all(0.0 < e <= b and b < 0.05 for e, b in zip(emu, bnd)), (name, dtype, emu, bnd)
        for seed in (1, 2):
            other = R.emulation_errors(name, dtype, seed)
            print(f"  seed {seed}: emulation {['%.3e' % e for e in other]}  of the bound {['%.3f' % (e / b) for e, b in zip(other, bnd)]}")
            assert all(0.0 < e <= b for e, b in zip(other, bnd)), (name, dtype, seed, other, bnd)


def test_mode_5_classes_follow_the_mix_bits():
    assert R.mode_of(5).classes == {"attn", "geglu", "qkv", "ff", "out1", "out2", "q2"}
    assert R.mode_of(5, 1 | 2 | 1024).classes == {"attn", "geglu"}      # the fallback classes are another arithmetic: the GPU test asserts the bits
    assert set(R.DEFECTS) == {"emb_slice_neighbour", "emb_other_entry", "skip_dropped", "one_scale", "norm_out_stats_in", "stale_ln_stats",
                              "ctx_other_entry", "ctx_pad_live", "vt_pad_nonzero", "geglu_swapped", "proj_out_no_residual", "dst_col0",
                              "rf/emb_slice_neighbour", "rf/stale_ln_stats", "rf/ctx_pad_live", "rf/vt_pad_nonzero", "rf/skip_dropped", "rf/dst_col0",
                              "rf/one_scale", "rf/splitk_slice_lost", "rf/splitk_tail_rows", "rf/head_width_128"}
    # a defect of the refiner plan is planted on a refiner case, and only there
    assert all((R.CONFIG_OF[name] == "refiner") == d.startswith("rf/") for d, (name, _) in R.DEFECTS.items())


@pytest.mark.parametrize("defect", list(R.DEFECTS))
def test_planted_defect_leaves_the_bound(defect):
    name, dtype = R.DEFECTS[defect]
    assert dtype in R.case_dtypes(name)
    bnd, _ = R.bounds(name, dtype)
    errs = R.errors(R.emulate(name, dtype, defect=defect), name, f16w=R.mode_of(dtype).f16w)
    print(f"unet_block_ref defect {defect} on {name} dtype {dtype}: error {['%.3e' % e for e in errs]}  bound {['%.3e' % b for b in bnd]}")
    assert max(e / b for e, b in zip(errs, bnd)) > 1.0, (defect, errs, bnd)
