"""tests/clip_layer_ref.py checked against the oracle and against itself on the CPU, on the very operands tests/test_gpu_clip_layer.py sends to the GPU:
the fp64 reference agrees with oracle/clip.py (fp32) on the same weights, the f32 emulation sits at fp32 level under fp64 and the f16-operand ones at
f16 level, every bound is finite and non-zero, and every planted defect lands at least 5 x outside the bound (margin x the emulation's own error
against fp64) of every case and mode it applies to.  So a GPU result inside those bounds rules the planted defects out.

The oracle agreement is held to 2e-5 of the branch (layer) / of max|pooled|: the oracle is one fp32 evaluation of the same chain, its rounding the
f32 emulation's class (2^-24 on stream values of ~30 against branches of ~5, fp32 sums up to K = 5120 long), which the f32 emulation is held to as well;
an architectural disagreement (mask, scale, activation, LayerNorm, EOT) is four orders above that.

Defects run at both widths on the smallest case they apply to and, at width 768, on every other case they apply to.  Each must land at least 5 x
outside the bound.  Measured here (error / bound of the defective emulation, the worst entry; the clean emulations sit at 1 / margin by construction):
  f32: scale_sqrt_c 3.6e4 ... 5.3e4, act_swapped 1.7e3 ... 2.6e3, every other defect 6.6e4 ... 2.2e6.
  f16_f32res: act_swapped 6.8 ... 9.2, scale_sqrt_c 151 ... 226, heads_rotated / mask_shifted / mask_off / pos_by_row 273 ... 605, vt_group_entry and
    key_tail_in_softmax 677 ... 825, the residual and head defects 426 ... 8.2e3.
  f16: scale_sqrt_c 13 ... 34, heads_rotated / mask_shifted / mask_off 26 ... 85, vt_group_entry / key_tail_in_softmax / pos_by_row 58 ... 380, the
    residual and head defects 286 ... 2.2e3 (the f16 stream's own rounding of the +-30 channels sets that mode's layer bound); act_swapped is not held
    there (0.7 ... 1.3 x, 2.0 with the attention knocked out: clip_layer_ref.applies says why) and is recorded by a test of its own."""
import math

import pytest
import torch

import clip_layer_ref as R
from oracle import clip as OCL, model as OM

MODES = tuple(R.MODES.values())
FACTOR = 5.0


def _smallest(defect, mode, width):
    names = [c[0] for c in R.CASES if width in c[4] and R.applies(defect, c[0], mode)]
    return min(names, key=lambda n: R.case(n)[1] * R.case(n)[2])


def _factor(defect, name, width, mode):
    wset = R.case(name)[5]
    e = R.emulate(name, width, wset, mode, defect)
    if wset == "head":
        errs, (bounds, _) = R.pooled_errors(e["pooled"], name, width, wset), R.pooled_bounds(name, width, wset, mode)
    else:
        errs, (bounds, _) = R.layer_errors(e["out"], name, width, wset), R.layer_bounds(name, width, wset, mode)
    return max(v / b for v, b in zip(errs, bounds))


@pytest.mark.parametrize("name,width", [(n, w) for n in ("pair_77", "short_9", "single_1", "pool_embed_dim", "pool_9x77") for w in R.case(n)[4]])
def test_reference_agrees_with_the_oracle(name, width):
    _, B, S, _, _, wset = R.case(name)
    H, quick = R.WIDTHS[width]
    cfg = OCL.CLIPConfig(B * S, width, R.embed_dim(name, width), H, R.N_CTX, 1, quick)
    ids = R.case_inputs(name, width)["ids"]
    r = R.ref(name, width, wset)
    W = OM.to_torch(R.model_weights(name, width, wset))
    assert set(W) == {s.name for s in OCL.clip_param_specs(cfg)}
    if wset == "head":
        h0, pooled = OCL.forward_hidden_pooled(cfg, W, ids, 0)
        e = max(R.pooled_errors(pooled, name, width, wset))
        assert (h0.double() - r["x"]).abs().max() <= 2.0 ** -23 * r["x"].abs().max()      # the embedding: one fp32 add
        assert torch.equal(r["out"], r["x"])                                                # head weights: the stream is the embedding
    else:
        e = max(R.layer_errors(OCL.forward_hidden(cfg, W, ids, 1), name, width, wset))
    print(f"{name} {width}: oracle (fp32) against the fp64 reference {e:.3e}")
    assert e < 2e-5


@pytest.mark.parametrize("width", list(R.WIDTHS))
def test_inputs_are_what_the_cases_need(width):
    for name in R.LAYER_CASES:
        r, c = R.ref(name, width, "full"), R.case_inputs(name, width)
        B, S = c["ids"].shape
        assert sorted(c["ids"].flatten().tolist()) == list(range(B * S))                   # a permutation of the rows
        if S >= 9:
            sd = float(r["scores"].std())
            assert 1.8 <= sd <= 3.2, (name, sd)                                             # peaked softmax rows: std about 2 ... 3
    c = R.case_inputs("pair_77", width)
    col = c["tok"].abs().mean(0)
    assert int((col > 10 * col.median()).sum()) == 2                                        # two outlier channels
    w = {k: v.double() for k, v in R.weights(width, "full").items()}
    y = R.ref("pair_77", width, "mlp_only")["x"]
    pre = R._ln64(y, w["mlp_ln.gamma"], w["mlp_ln.beta"]) @ w["mlp.fc1.weight"] + w["mlp.fc1.bias"]
    assert float(pre.max()) > 5.0 and float(pre.min()) < -5.0                               # both tails of the activation
    for name in R.POOL_CASES:
        if width not in R.case(name)[4]:
            continue
        ids = R.case_inputs(name, width)["ids"]
        eot = R.first_argmax(ids)
        assert {b: int(eot[b]) for b in range(ids.shape[0])} == R.POOL_EOT[name]
        for b, t in R.POOL_TIES[name].items():
            assert t > int(eot[b]) and int(ids[b, t]) == int(ids[b].max())
    eots = set(R.POOL_EOT["pool_9x77"].values())
    assert {0, 76} <= eots and any(0 < e < 76 for e in eots)


@pytest.mark.parametrize("name,width", [(c[0], w) for c in R.CASES for w in c[4]])
def test_emulations_are_in_their_class_and_bounds_are_finite(name, width):
    _, B, S, _, _, wset = R.case(name)
    worst = {}
    for mode in MODES:
        a, b = R.emulate(name, width, wset, mode), R.emulate(name, width, wset, mode)
        assert all(torch.equal(a[k], b[k]) and torch.isfinite(a[k]).all() for k in a), "the emulation is a function of its operands"
        bounds, e = R.pooled_bounds(name, width, wset, mode) if wset == "head" else R.layer_bounds(name, width, wset, mode)
        assert len(bounds) == B and all(0.0 < v < math.inf for v in bounds), (name, mode, bounds)
        worst[mode] = max(e)
        print(f"{name} {width} {mode}: emulation against fp64 {', '.join(f'{v:.3e}' for v in e)} per entry")
        if wset == "head":
            assert torch.equal(a["out"], a["x"])
    # the classes: f32 at fp32 rounding of the chain; the f16-operand modes at operand rounding (2^-11 per operand, 2^-7 absolute on the outlier channels)
    assert worst["f32"] < 2e-5
    assert 20 * worst["f32"] < worst["f16_f32res"] < 2e-2 and 20 * worst["f32"] < worst["f16"] < 2e-2


@pytest.mark.parametrize("wset", ["attn_only", "mlp_only"])
@pytest.mark.parametrize("width", list(R.WIDTHS))
def test_knocked_out_branches_have_bounds_of_their_own(width, wset):
    for name in ("pair_77", "short_9"):
        for mode in MODES:
            bounds, e = R.layer_bounds(name, width, wset, mode)
            assert all(0.0 < v < math.inf for v in bounds)
            print(f"{name} {width} {wset} {mode}: emulation against fp64 {', '.join(f'{v:.3e}' for v in e)} per entry")
            assert max(e) < (2e-5 if mode == "f32" else 2e-2)


HELD = [(d, m) for d in R.DEFECTS for m in MODES if any(R.applies(d, c[0], m) for c in R.CASES)]


@pytest.mark.parametrize("defect,mode", HELD)
def test_defects_leave_the_bounds(defect, mode):
    for width in R.WIDTHS:
        first = _smallest(defect, mode, width)
        names = [first] + [c[0] for c in R.CASES if width == 768 and c[0] != first and R.applies(defect, c[0], mode)]
        for name in names:
            r = _factor(defect, name, width, mode)
            print(f"{defect} {name} {width} {mode}: {r:.3g} x bound")
            assert r >= FACTOR, (defect, name, width, mode, r)


def test_act_swapped_in_f16_is_recorded():
    # the one (defect, mode) pair that is not held (clip_layer_ref.applies says why): its factors, for the record
    assert ("act_swapped", "f16") not in HELD and ("act_swapped", "f16_f32res") in HELD and ("act_swapped", "f32") in HELD
    for width in R.WIDTHS:
        for name, wset in [(n, "full") for n in R.LAYER_CASES] + [("pair_77", "mlp_only"), ("short_9", "mlp_only")]:
            e = R.layer_errors(R.emulate(name, width, wset, "f16", "act_swapped")["out"], name, width, wset)
            r = max(v / b for v, b in zip(e, R.layer_bounds(name, width, wset, "f16")[0]))
            print(f"act_swapped {name} {width} {wset} f16 (not held): {r:.3g} x bound")
            assert math.isfinite(r)


def test_applies_tables_hide_nothing():
    # every defect is held in the modes it names at both widths, and names every mode but the one documented exception
    assert set(HELD) == {(d, m) for d in R.DEFECTS for m in MODES} - {("act_swapped", "f16")}
    for defect, mode in HELD:
        for width in R.WIDTHS:
            assert any(R.applies(defect, c[0], mode) for c in R.CASES if width in c[4]), (defect, mode, width)
    # a defect that cannot show at a shape leaves the clean bits there: what applies() says about shapes is what the emulation does
    clean = R.emulate("exact_64", 768, "full", "f16")
    for defect in ("vt_group_entry", "key_tail_in_softmax", "pos_by_row", "eot_last"):
        assert not R.applies(defect, "exact_64", "f16")
        d = R.emulate("exact_64", 768, "full", "f16", defect) if defect != "pos_by_row" else None
        assert d is None or (torch.equal(d["out"], clean["out"]) and torch.equal(d["pooled"], clean["pooled"])), defect
    one = R.emulate("single_1", 768, "full", "f32")
    for defect in ("mask_shifted", "mask_off", "heads_rotated", "scale_sqrt_c"):
        assert not R.applies(defect, "single_1", "f32") and torch.equal(R.emulate("single_1", 768, "full", "f32", defect)["out"], one["out"])


def test_embedding_expectation_is_the_stored_sum():
    c = R.case_inputs("short_9", 768)
    ids = c["ids"]
    for mode in MODES:
        e = R.embed_expected(c["tok"], c["pos"], ids, mode)
        assert torch.equal(e[1, 3], R._sd(mode, R._cd(mode, c["tok"][ids[1, 3]]) + R._cd(mode, c["pos"][3])))
        assert torch.equal(e, R.f16(e)) == (mode == "f16")      # only the f16 stream is rounded after the add
    assert torch.equal(R.embed_expected(c["tok"], c["pos"], ids, "f32"), c["tok"][ids] + c["pos"][:9])
