"""The weight packing, bit for bit: every case of tests/golden/weight_pack_bits.npz again -- what the packed weights compute (SHA-256 of every output),
the arena bytes, the MixClass bits in force, whether a shadow was taken.

The fixture was recorded from the commit before WeightBuilder's six projection routines became one (tools/record_weight_pack_fixture.py; cases and
layout in tests/weight_pack_cases.py).  A case that fails here means a packed byte, an arena offset or a packing decision changed: read
WeightBuilder::pack / conv, never re-record."""
import os

import numpy as np
import pytest

import weight_pack_cases as C

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_pack_bits.npz")
GOLDEN = C.load(FIXTURE)


@pytest.mark.parametrize("case", C.all_cases(), ids=C.case_name)
def test_case_equals_the_record(pkg, ctx, case):
    name = C.case_name(case)
    want_outs, want_ints = C.recorded(GOLDEN, case)
    assert want_ints or want_outs, f"{name} is not in the fixture"
    outs, ints = C.run_case(pkg, ctx, case)
    assert ints == want_ints, name
    assert sorted(outs) == sorted(want_outs), name
    for k, (sha, sample) in outs.items():
        ref_sha, ref_sample = want_outs[k]
        d = np.abs(sample.astype(np.float64) - ref_sample.astype(np.float64))
        assert sha == ref_sha, f"{name}/{k}: digest differs; of the 256 sampled values {int((d > 0).sum())} differ, max-abs {d.max():.3e} (max |ref| {np.abs(ref_sample).max():.3e})"
