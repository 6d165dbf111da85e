"""tests/golden/sampler_step_bits.npz read alone: is the case matrix complete, and is every axis of it live in what was recorded.

A fixture whose cases agree with each other would pin nothing: two cases that differ in exactly one of solver, eta, guidance form or inpainting must
have different final latents.  The storage type of the UNet-input copy never reaches the latent (the state is fp32; only the copy is rounded), so that
axis is held to the copy instead.  Explicit noise against seeded noise at eta 0 is no axis without inpainting (nothing is drawn: equal latents, and
that is asserted too); with inpainting the blend noise differs."""
import itertools
import os

import numpy as np
import pytest

import sampler_step_cases as C

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_step_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _latent(golden, c):
    return C.unpack(c, golden["out/" + C.case_name(c)])[0]


def test_file_is_small_and_says_where_it_came_from(golden):
    assert os.path.getsize(FIXTURE) < 1_000_000
    meta = C.load_meta(golden)
    assert len(meta["parent_commit"]) >= 7 and "version" in meta["hipcc"].lower()
    assert meta["cases"] == [C.case_name(c) for c in C.all_cases()]


def test_matrix_is_complete(golden):
    main = C.matrix()
    assert len(main) == 2 * 3 * 5 * 2 and len({C.case_name(c) for c in main}) == 60
    assert {(c["solver"], c["noise"], c["guidance"], c["inpaint"]) for c in main} == \
        set(itertools.product(("ddim", "dpmpp_2m"), ("explicit", "seeded0", "seeded07"), ("scalar", "single", "scales", "interval", "all"), (False, True)))
    assert all(c["shape"] == (2, 8, 17) and c["schedule"] == "s4" and not c["input_f16"] for c in main)
    side = C.side_cases()
    for solver in C.SOLVERS:
        mine = [c for c in side if c["solver"] == solver]
        assert all(c["noise"] == "seeded07" and c["inpaint"] for c in mine)
        assert {c["shape"] for c in mine} == {(1, 8, 8), (2, 8, 17), (3, 8, 12)}
        assert any(c["schedule"] == "refiner" for c in mine) and any(c["input_f16"] for c in mine)
    for c in C.all_cases():
        name, (n, h, w) = C.case_name(c), c["shape"]
        B = n if c["guidance"] == "single" else 2 * n
        rec = golden["out/" + name]
        assert rec.dtype == np.float32 and rec.shape == (n + B + (n if c["solver"] == "dpmpp_2m" else 0), 4, h * w), name
        assert np.isfinite(rec).all(), name
        assert golden["sha/" + name].shape == (2,) and all(len(str(v)) == 64 for v in golden["sha/" + name]), name
    for shape in C.SHAPES:
        n, h, w = shape
        k = f"in/{C.shape_key(shape)}/"
        assert golden[k + "eps"].shape == (C.MAX_ITERS, 2 * n, h * w, 4) and golden[k + "step_noise"].shape == (C.MAX_ITERS, n, 4, h, w)
        assert golden[k + "seeds"].dtype == np.uint64 and golden[k + "mask"].dtype == np.uint8
        for b in range(n):
            assert set(np.unique(golden[k + "mask"][b])) == {0, 1}


def test_interval_leaves_iterations_on_both_sides():
    ts = [999, 749, 499, 249]
    active = [C.T_RANGE[0] <= t <= C.T_RANGE[1] for t in ts]
    assert any(active) and not all(active)


@pytest.mark.parametrize("axis", ["solver", "noise", "guidance", "inpaint"])
def test_axis_is_live_in_the_latents(golden, axis):
    main = C.matrix()
    pairs = 0
    for a, b in itertools.combinations(main, 2):
        if a[axis] == b[axis] or any(a[k] != b[k] for k in C.AXES if k != axis):
            continue
        same = np.array_equal(_latent(golden, a), _latent(golden, b))
        if axis == "noise" and {a["noise"], b["noise"]} == {"explicit", "seeded0"} and not a["inpaint"]:
            assert same, f"nothing is drawn, yet {C.case_name(a)} and {C.case_name(b)} differ"
        else:
            assert not same, f"{C.case_name(a)} and {C.case_name(b)} were recorded with equal final latents"
        pairs += 1
    assert pairs == {"solver": 30, "noise": 60, "guidance": 120, "inpaint": 30}[axis]


def test_input_type_is_live_in_the_copy(golden):
    for c in C.side_cases():
        if c["input_f16"]:
            lat16, in16, _ = C.unpack(c, golden["out/" + C.case_name(c)])
            lat32, in32, _ = C.unpack(dict(c, input_f16=False), golden["out/" + C.case_name(dict(c, input_f16=False))])
            assert np.array_equal(lat16, lat32)
            assert not np.array_equal(in16, in32)
            assert np.array_equal(in16, in32.astype(np.float16).astype(np.float32))       # the copy is the latent rounded to f16, to nearest even
            assert np.array_equal(in32, np.concatenate([lat32, lat32]))                   # and, as f32, the latent itself, once per branch


def test_shape_and_schedule_cases_are_their_own(golden):
    for c in C.side_cases():
        if c["schedule"] == "refiner":
            assert not np.array_equal(_latent(golden, c), _latent(golden, dict(c, schedule="s4")))


def test_rescale_is_live_against_its_partner(golden):
    for p in C.partner_cases():
        with_rescale = dict(p, guidance="all")
        assert not np.array_equal(_latent(golden, p), _latent(golden, with_rescale))
        # entry 1 runs scale 7.5 on the active iterations in both, so only the factor separates the two records of that entry
        assert not np.array_equal(_latent(golden, p)[1], _latent(golden, with_rescale)[1])
