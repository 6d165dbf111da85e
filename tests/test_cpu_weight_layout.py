"""The weight arenas are sized by a layout pass (the model's loader over a dry arena and an empty source, csrc/weights.cpp WeightBuilder): through
sdxl_debug_weight_layout that pass must return, without a GPU, the arena bytes tests/golden/weight_pack_bits.npz recorded from created models of
the commit before it existed -- every full-size entry (the weight broadcast's sizes) and every tiny model the GPU cases run.  A byte more or less
means an allocation of WeightBuilder::pack / conv / norm or of a loader changed: replicas would no longer receive rank 0's arena."""
import ctypes
import os

import pytest

import weight_pack_cases as C

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_pack_bits.npz")
GOLDEN = C.load(FIXTURE)
LAYOUT_CASES = [c for c in C.all_cases() if "arena_bytes" in C.recorded(GOLDEN, c)[1]]


@pytest.fixture(scope="module")
def built(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg


def test_fixture_is_complete():
    meta = C.load_meta(GOLDEN)
    names = [C.case_name(c) for c in C.all_cases()]
    assert len(set(names)) == len(names)
    assert sorted(meta["cases"] + meta["not_reproduced"]) == sorted(names) and 10 * len(meta["not_reproduced"]) <= len(names)
    assert len(meta["parent_commit"]) == 40 and "version" in meta["hipcc"].lower() and meta["build_info"]
    # cases 6, 1, 4, 5 of the record: 16 + 6 full-size entries, 22 UNets, 6 VAEs, 6 CLIP towers
    assert len(LAYOUT_CASES) == 22 + 22 + 6 + 6
    assert os.path.getsize(FIXTURE) < 400 * 1024


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=C.case_name)
def test_layout_pass_returns_the_recorded_bytes(built, case):
    pkg = built
    ints = C.recorded(GOLDEN, case)[1]
    _, cfg, dtype, option = C.layout_query(pkg, case, ints)
    assert pkg.weight_layout_bytes(cfg, dtype, option) == ints["arena_bytes"]


def test_argument_errors(built):
    pkg = built
    n = ctypes.c_size_t(0)
    u, v = pkg.sdxl_base_config().to_c(), pkg.VAEConfig().to_c()
    entry = pkg.lib().sdxl_debug_weight_layout
    assert entry(None, None, None, 1, 0, ctypes.byref(n)) != 0                          # no model
    assert entry(ctypes.byref(u), ctypes.byref(v), None, 1, 0, ctypes.byref(n)) != 0    # two
    assert entry(ctypes.byref(u), None, None, 1, -1, None) != 0                         # nowhere to write
    assert entry(ctypes.byref(u), None, None, 99, -1, ctypes.byref(n)) != 0             # unknown dtype
    assert entry(None, ctypes.byref(v), None, 5, 0, ctypes.byref(n)) != 0               # a UNet-only mode
    assert entry(ctypes.byref(u), None, None, 1, -1, ctypes.byref(n)) == 0 and n.value > 0
