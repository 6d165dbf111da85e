"""Create-time adapters, host side (no GPU): sdxl_lora_check on the base config, the binding's layout rule, and the five new symbols in
the header and in the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import config as OC
from util import to_pkg_cfg
import lora_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LORA_SYMBOLS = ("sdxl_lora_check", "sdxl_lora_merge", "sdxl_unet_create_lora", "sdxl_diffuser_create_lora")


@pytest.fixture(scope="module")
def built(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg


@pytest.fixture(scope="module")
def base(built):
    cfg = built.sdxl_base_config()
    return cfg, built.unet_param_specs(cfg)


def _entry(built, specs, name, rank=4):
    """a valid entry on parameter `name`: zeros of the right extents"""
    i = built.param_index(specs, name)
    shape = specs[i].shape
    if specs[i].kind == 1:
        down, up = np.zeros((rank,) + tuple(shape[1:]), np.float32), np.zeros((shape[0], rank), np.float32)
    else:
        down, up = np.zeros((rank, shape[0]), np.float32), np.zeros((shape[1], rank), np.float32)
    return built.lora_entry(i, down, up)


def test_header_declares_and_library_exports_the_lora_symbols(built):
    hdr = open(os.path.join(ROOT, "include", "sdxl_mi355.h")).read()
    declared = set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", hdr))
    l = ctypes.CDLL(built.LIB_PATH)
    for s in LORA_SYMBOLS:
        assert s in declared, s
        assert s in built.ABI_SYMBOLS, s
        assert hasattr(l, s), s
    assert re.search(r"\}\s*sdxl_lora_entry\s*;", hdr) and "SDXL_LORA_ROUND_F16 = 1" in hdr      # the fifth: the entry type (+ its flag)
    assert ctypes.sizeof(built.LoraEntry) == 32 and built.LoraEntry.left.offset == 8 and built.LoraEntry.right.offset == 16 \
        and built.LoraEntry.scale.offset == 24      # { int32 param_index, rank; const float* left, *right; float scale; } on LP64
    assert built.LORA_ROUND_F16 == 1


def test_lora_check_accepts_a_valid_list(built, base):
    cfg, specs = base
    names = ["input_blocks.4.transformer.blocks.0.attn1.query.weight", "input_blocks.4.transformer.blocks.0.attn2.key.weight",
             "middle_block.transformer.blocks.9.mlp.geglu.proj.weight", "output_blocks.0.res.conv_in.weight", "lin2_time_embed.weight",
             "input_blocks.4.transformer.blocks.0.attn1.query.weight"]      # (the same tensor twice: adapters stack)
    built.lora_check(cfg, [_entry(built, specs, n) for n in names])
    built.lora_check(cfg, [])
    assert built.lib().sdxl_lora_check(ctypes.byref(cfg.to_c()), None, 0) == 0


def test_lora_check_rejects_each_fault_with_its_own_message(built, base):
    cfg, specs = base
    good = "input_blocks.4.transformer.blocks.0.attn1.query.weight"
    msgs = []

    def refused(entry, *words):
        with pytest.raises(built.InvalidArgument) as ei:
            built.lora_check(cfg, [_entry(built, specs, good), entry])
        m = str(ei.value)
        assert "entry 1" in m and all(w in m for w in words), m
        msgs.append(m)

    for bad_index in (len(specs), -1):
        e = _entry(built, specs, good); e.param_index = bad_index
        refused(e, "out of range")
    for name in ("input_blocks.4.transformer.blocks.0.attn1.out.bias", "input_blocks.4.transformer.blocks.0.norm1.gamma",
                 "input_blocks.4.transformer.blocks.0.norm1.beta", "input_blocks.4.transformer.blocks.0.norm1.eps"):
        e = _entry(built, specs, good); e.param_index = built.param_index(specs, name)
        refused(e, "not a LINEAR_W / CONV_W parameter", name)
    e = _entry(built, specs, good); e.rank = 0
    refused(e, "rank")
    for field in ("left", "right"):
        e = _entry(built, specs, good); setattr(e, field, None)
        refused(e, "NULL")
    for v in (float("nan"), float("inf"), float("-inf")):
        e = _entry(built, specs, good); e.scale = v
        refused(e, "scale", "finite")
    # five kinds of fault, five different texts (the entry number and parameter name aside)
    kinds = {re.sub(r"'[^']*'|-?\d+", "", m) for m in msgs}
    assert len(kinds) == 5, kinds
    rc = built.lib().sdxl_lora_check(ctypes.byref(cfg.to_c()), None, 2)
    assert rc == 1 and b"NULL" in built.lib().sdxl_last_error()
    assert built.lib().sdxl_lora_check(None, None, 0) == 1


def test_lora_entry_layout_rule(built):
    # Linear [d_in, d_out]: left = down^T, right = up^T; Conv [Cout, Cin, kh, kw]: left = up, right = down flattened; scale = strength alpha / r
    ocfg = OC.tiny_config()
    specs = built.unet_param_specs(to_pkg_cfg(built, ocfg))
    rng = np.random.default_rng(0)
    i = LR.find(specs, ".attn1.query.weight")
    d_in, d_out = specs[i].shape
    down, up = rng.standard_normal((3, d_in)).astype(np.float32), rng.standard_normal((d_out, 3)).astype(np.float32)
    e = built.lora_entry(i, down, up, alpha=6.0, strength=0.5)
    assert (e.param_index, e.rank, e.scale) == (i, 3, 1.0)
    assert np.array_equal(e.keep[0], down.T) and np.array_equal(e.keep[1], up.T) and e.keep[0].flags.c_contiguous and e.keep[1].flags.c_contiguous
    assert e.left == e.keep[0].ctypes.data and e.right == e.keep[1].ctypes.data
    assert built.lora_entry(i, down, up).scale == 1.0      # alpha defaults to the rank
    j = LR.find(specs, ".conv_in.weight")
    cout, cin, kh, kw = specs[j].shape
    cdown, cup = rng.standard_normal((2, cin, kh, kw)).astype(np.float32), rng.standard_normal((cout, 2, 1, 1)).astype(np.float32)
    c = built.lora_entry(j, cdown, cup)
    assert np.array_equal(c.keep[0], cup.reshape(cout, 2)) and np.array_equal(c.keep[1], cdown.reshape(2, cin * kh * kw))
    le, ri = LR.left_right(specs[i], down, up)
    assert np.array_equal(le, e.keep[0]) and np.array_equal(ri, e.keep[1])      # the tests' own restatement agrees
    with pytest.raises(built.EngineError):
        built.lora_entry(i, down, up[:, :2])
    with pytest.raises(built.EngineError):
        built.param_index(specs, "no.such.weight")
